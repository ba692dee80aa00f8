"""Every call that turns a row of logits into a token id, on rows that hold a NaN, an infinity, a signed zero or a
denormal.

THE RULE (csrc/argmax_rule.h) is the reference's scan (main.zig:715-726: max = x[0], then strict '>'): index
0 if x[0] is a NaN, otherwise the lowest index of the largest non-NaN value, index 0 if there is none.  The expected id is
always first_strict_max(row), a transcription of that scan -- never np.argmax (which takes a NaN for the maximum) and
never a kernel's answer.  At a temperature the expected id is the host sampler's on l2z_probs_read's probabilities, which
on such rows are all NaN.

Hook-fed rows reach the scans of a logits vector (argmax_kernel's two paths, block_argmax_1024); model-fed rows -- a
one-layer checkpoint whose classifier row i is the constant v[i], so every row of every call has the same logits --
reach the fused classifier epilogue, wide_logits_out, the verify family's verdicts and l2z_score's top-1.  All families
must return ONE id on a case: the plain greedy loop and a speculative one must emit the same sequence.  Every logits row
a call exposes is first held to the planted pattern -- NaN and +-inf exactly at the planted classifier rows -- which is how
these tests found the short-prompt GEMM reading a NaN weight of a later row into the rows before it.
"""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_parity import LOGIT_ATOL, LOGIT_RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "llama2.zig_amd", "host")
NAN, INF = np.float32(np.nan), np.float32(np.inf)
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
HOOK_VOCABS = (1000, 5003, 8200, 32000)


def first_strict_max(x):
    """main.zig:715-726 on f32 values"""
    x = np.asarray(x, np.float32)
    best, at = x[0], 0
    for i in range(1, x.size):
        if x[i] > best:      # False whenever either side is a NaN
            best, at = x[i], i
    return at


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_row(V, k, frac):
    """(row, indices of the duplicated maximum): seeded normal values, the maximum at three drawn indices, then `frac` of
    the positions (drawn over the whole row, the maxima and index 0 included) replaced by NaN"""
    rng = np.random.default_rng([V, k, int(frac * 100)])
    x = rng.standard_normal(V, dtype=np.float32)
    dup = np.sort(rng.choice(V, 3, replace=False))
    x[dup] = np.float32(x.max() + 1.0)
    x[rng.choice(V, int(V * frac), replace=False)] = NAN
    return x, dup


def hook_rows(V):
    """name -> row of V logits; zeros except as named"""
    def zeros(**at):
        x = np.zeros(V, np.float32)
        for i, v in at.items():
            x[int(i[1:])] = v
        return x
    rows = {"nan5_max37": zeros(_5=NAN, _37=1.0)}
    if V > 1029:
        rows["nan5_max1029"] = zeros(_5=NAN, _1029=1.0)
    rows["nan4_max6"] = zeros(_4=NAN, _6=1.0)
    rows["nan0_max500"] = zeros(_0=NAN, _500=1.0)
    x = np.full(V, NAN, np.float32); x[700] = 3.0
    rows["all_nan_but_700"] = x
    rows["all_nan"] = np.full(V, NAN, np.float32)
    x = np.full(V, NAN, np.float32); x[0] = -1.5
    rows["finite0_nan_rest"] = x
    x = np.zeros(V, np.float32); x[[70, V - 1]] = INF
    rows["pinf_70_and_last"] = x
    x = np.zeros(V, np.float32); x[0] = -0.0
    rows["negzero_first"] = x
    x = np.full(V, -0.0, np.float32); x[0] = 0.0
    rows["poszero_first"] = x
    x = np.full(V, -INF, np.float32); x[3] = NAN
    rows["neginf_nan3"] = x
    rows["denormals"] = zeros(_777=1e-45, _900=3e-45)
    for k in range(4):
        rows[f"rand_nan1pct_{k}"] = random_row(V, k, 0.01)[0]
    for k in range(4):
        rows[f"rand_nan50pct_{k}"] = random_row(V, k, 0.50)[0]
    return rows


# what the scan returns on every hook-fed row, written out (test_the_transcription_is_the_oracles_scan holds
# first_strict_max and the oracle to it)
FIXED_WANT = {"nan5_max37": 37, "nan5_max1029": 1029, "nan4_max6": 6, "nan0_max500": 0, "all_nan_but_700": 0, "all_nan": 0,
              "finite0_nan_rest": 0, "pinf_70_and_last": 70, "negzero_first": 0, "poszero_first": 0, "neginf_nan3": 0,
              "denormals": 900}
RANDOM_WANT = {   # vocabulary -> ids of rand_nan1pct_0..3, rand_nan50pct_0..3
    1000: (162, 25, 354, 120, 0, 0, 0, 749),     # (0: the row drew a NaN for index 0)
    5003: (887, 3154, 2370, 3536, 0, 831, 0, 0),
    8200: (1350, 1990, 804, 1704, 0, 0, 0, 0),
    32000: (11774, 1984, 12811, 3310, 13551, 0, 0, 12661),
}


def hook_want(V, name):
    if name in FIXED_WANT:
        return FIXED_WANT[name]
    kind, k = name.rsplit("_", 1)
    return RANDOM_WANT[V][int(k) + (4 if kind == "rand_nan50pct" else 0)]


@pytest.mark.parametrize("V", HOOK_VOCABS)
def test_the_transcription_is_the_oracles_scan(orc, V):
    rows = hook_rows(V)
    assert len(rows) == (20 if V > 1029 else 19)
    for name, x in rows.items():
        assert first_strict_max(x) == orc.argmax(x) == hook_want(V, name), name
    assert np.isnan(rows["denormals"]).sum() == 0 and 0 < rows["denormals"][777] < rows["denormals"][900] < 1e-44
    for k in range(4):   # the random rows hold what they are meant to hold
        for frac in (0.01, 0.50):
            x, dup = random_row(V, k, frac)
            assert int(np.isnan(x).sum()) == int(V * frac)
            keep = dup[~np.isnan(x[dup])]
            if keep.size and not np.isnan(x[0]):
                assert first_strict_max(x) == keep[0] and np.all(bits(x[keep]) == bits(x[keep[0]]))


# ---------------------------------------------------------------------------------------------------------- hook-fed
def hook_cfg(ck, V):
    return ck.Config(dim=64, hidden_dim=172, n_layers=1, n_heads=4, n_kv_heads=2, vocab_size=V, seq_len=16)


@pytest.mark.gpu
@pytest.mark.parametrize("V", HOOK_VOCABS)
def test_hook_fed_pickers_follow_the_scan(gpu, ck, V):
    """gpu.argmax (argmax_kernel on a vector: the float4 path where V is a multiple of 4, else the scalar one),
    write_logits + l2z_argmax, l2z_argmax_batch on 1, 2 and 16 runstates and l2z_sample_batch at temperature 0
    (block_argmax_1024), on every row of hook_rows; no call changes a bit of the logits."""
    cfg = hook_cfg(ck, V)
    rows = hook_rows(V)
    names = list(rows)
    want = {n: first_strict_max(rows[n]) for n in names}
    states = [gpu.RunState(cfg) for _ in range(16)]
    wrong = []

    def note(picker, name, got):
        print(f"V {V} {name}: {picker} -> {int(got)}, the scan {want[name]}")
        if int(got) != want[name]:
            wrong.append((name, picker, int(got), want[name]))

    def unchanged(held):
        for s, n in zip(states, held):
            assert np.array_equal(bits(s.logits()), bits(rows[n])), f"{n}: the logits changed"

    for start in (0, len(names) - 16):   # two rounds of 16 different rows cover the list
        held = names[start:start + 16]
        for s, n in zip(states, held):
            s.write_logits(rows[n])
        unchanged(held)
        for n in held:
            note("argmax(x)", n, gpu.argmax(rows[n]))
        for s, n in zip(states, held):
            note("write_logits + argmax", n, s.argmax())
        unchanged(held)
        for cnt in (1, 2, 16):
            for n, got in zip(held, gpu.argmax_batch(states[:cnt])):
                note(f"argmax_batch of {cnt}", n, got)
            unchanged(held)
        for n, got in zip(held, gpu.sample_batch(states, 0.0, 0.9, 0.5)):
            note("sample_batch at temperature 0", n, got)
        unchanged(held)
    for s in states:
        s.close()
    assert not wrong, f"(row, picker, got, the scan): {wrong}"


# ---------------------------------------------------------------------------------------------------------- model-fed
PINF_W, NINF_W = np.float32(3e38), np.float32(-3e38)   # x is rmsnorm(ones): every one of the 64 products overflows


def planted(V, case):
    """classifier constants v[0 .. V): 1.0, 2.0 at the tied maximum, NaN, +-3e38 for +-inf"""
    v = np.ones(V, np.float32)
    if case == "nan5_max37":
        v[5], v[37] = NAN, 2.0
    elif case == "nan4_max6":
        v[4], v[6] = NAN, 2.0
    elif case == "nan5_max1029":
        v[5], v[1029] = NAN, 2.0
    elif case == "nan0_max500":
        v[0], v[500] = NAN, 2.0
    elif case == "all_nan_but_700":
        v[:] = NAN
        v[700] = 2.0
    elif case == "pinf_70_and_last":
        v[[70, V - 1]] = PINF_W
    elif case == "neginf_segment":    # one whole segment of score.hip
        v[:4096] = NINF_W
        v[[4099, V - 1]] = 2.0
    elif case == "neginf_wave":       # one wave's share of a 1024-column scan
        v[:256] = NINF_W
        v[[259, V - 1]] = 2.0
    else:                             # the NaN mask of a random 1 % row over a tied-maximum row
        x, dup = random_row(V, int(case[-1]), 0.01)
        v[dup] = 2.0
        v[np.isnan(x)] = NAN
    return v


# case -> (the scan's id, an id a kernel of the parent commit returned instead or None)
MODEL_CASES = {
    1024: {"nan5_max37": (37, 0), "nan4_max6": (6, 0), "nan0_max500": (0, 500), "all_nan_but_700": (0, 700),
           "pinf_70_and_last": (70, None), "neginf_wave": (259, None), "mask_0": (50, None), "mask_1": (19, None)},
    32000: {"nan5_max37": (37, 0), "nan4_max6": (6, 0), "nan5_max1029": (1029, 0), "nan0_max500": (0, 500),
            "all_nan_but_700": (0, 700), "pinf_70_and_last": (70, None), "neginf_segment": (4099, None),
            "mask_0": (11774, None), "mask_1": (1984, None)},
}
MODEL_PARAMS = [(V, c) for V in MODEL_CASES for c in MODEL_CASES[V]]


def check_pattern(lg, v, where):
    """the logits row is what the planted constants say: NaN and +-inf exactly there, the tied rows bit-equal and above
    every other finite value"""
    assert np.array_equal(np.isnan(lg), np.isnan(v)), f"{where}: NaN off the planted rows"
    assert np.array_equal(np.isposinf(lg), v == PINF_W), f"{where}: +inf off the planted rows"
    assert np.array_equal(np.isneginf(lg), v == NINF_W), f"{where}: -inf off the planted rows"
    tied, plain = np.flatnonzero(v == 2.0), np.flatnonzero(v == 1.0)
    if tied.size:
        assert np.all(bits(lg[tied]) == bits(lg[tied[0]])), f"{where}: the tied rows differ"
        assert plain.size == 0 or lg[tied[0]] > lg[plain].max(), f"{where}: the tied rows are not the maximum"


def make_model(gpu, ck, V, v, n_kv_heads):
    cfg = ck.Config(dim=64, hidden_dim=172, n_layers=1, n_heads=4, n_kv_heads=n_kv_heads, vocab_size=V, seq_len=96)
    blob = ck.synth_blob(cfg, False, 21)
    t = {d.name: d for d in ck.tensor_table(cfg, False)}

    def fill(name, value):
        blob[t[name].offset:t[name].offset + t[name].count] = value

    fill("token_embedding_table", 1.0); fill("wo", 0.0); fill("w2", 0.0); fill("rms_final_weight", 1.0)
    fill("wcls", np.repeat(v, cfg.dim))
    return cfg, gpu.Weights(cfg, blob, False)


def close(objs):
    for o in objs:
        o.close()


@pytest.fixture(scope="module")
def H(B):
    L = C.CDLL(os.path.join(HOST, "libllama2_host.so"))
    fp = C.POINTER(C.c_float)
    L.l2zh_sample_coin.restype = C.c_size_t
    L.l2zh_sample_coin.argtypes = [fp, C.c_size_t, C.c_float]
    L.l2zh_sample_top_p_coin.restype = C.c_size_t
    L.l2zh_sample_top_p_coin.argtypes = [fp, C.c_size_t, C.c_float, C.c_float, fp]
    return L


def host_token(H, probs, top_p, coin):
    assert np.isnan(probs).all(), "the case is about all-NaN probabilities"
    pp = probs.ctypes.data_as(C.POINTER(C.c_float))
    if top_p in (0.0, 1.0):
        return int(H.l2zh_sample_coin(pp, probs.size, C.c_float(coin)))
    return int(H.l2zh_sample_top_p_coin(pp, probs.size, C.c_float(top_p), C.c_float(coin), None))


@pytest.mark.gpu
@pytest.mark.parametrize("x3", [1, 2], ids=["x3_1", "x3_2"])
@pytest.mark.parametrize("V,case", MODEL_PARAMS, ids=[f"{V}-{c}" for V, c in MODEL_PARAMS])
def test_every_family_picks_the_scans_token(gpu, ck, options, V, case, x3):
    """One checkpoint, one logits row everywhere, every family's ids in one list: all equal, and the scan's."""
    v = planted(V, case)
    cfg4, w4 = make_model(gpu, ck, V, v, 4)   # the fused small-model path (stepped and greedy entries)
    cfg, w = make_model(gpu, ck, V, v, 2)     # (both made under the default options)
    options(L2Z_PF_X3=x3)
    ids = {}   # family -> every id it returned

    # ---- the stepped pass: the row every other one is held to
    s, s2 = gpu.RunState(cfg4), gpu.RunState(cfg4)
    s.transformer(1, 0, w4)
    lg = s.logits()
    check_pattern(lg, v, "l2z_transformer")
    want = first_strict_max(lg)
    literal, parent_id = MODEL_CASES[V][case]
    assert want == literal
    wrong = parent_id if parent_id is not None else (want + 1) % V   # any other id must be refused as a guess

    bad_rows = []   # the calls whose logits are not the planted pattern (all of them named before the test fails)

    def row(lgr, where):
        try:
            check_pattern(lgr, v, where)
            assert first_strict_max(lgr) == want, where
        except AssertionError as e:
            bad_rows.append(str(e).split("\n")[0])

    ids["transformer + argmax (fused candidates)"] = [s.argmax()]
    s2.write_logits(lg)
    ids["write_logits + argmax"] = [s2.argmax()]
    s.greedy_begin([])
    ids["greedy_run"] = s.greedy_run(w4, 2).tolist()
    s.greedy_begin([])
    ids["sample_run at temperature 0"] = s.sample_run(w4, 2, 0.0, 1.0, None).tolist()
    assert len(ids["greedy_run"]) == 2 and len(ids["sample_run at temperature 0"]) == 2   # (no case's id is BOS)
    close([s, s2])

    # ---- prompt pass, batched and wide steps
    s = gpu.RunState(cfg)
    s.prefill([1, 2, 3, 4, 5], 0, w)
    row(s.logits(), "l2z_prefill")
    ids["prefill + argmax"] = [s.argmax()]
    s.close()
    states = [gpu.RunState(cfg) for _ in range(33)]
    gpu.transformer_batch(states[:3], [1, 2, 3], [0, 0, 0], w)
    row(states[2].logits(), "l2z_transformer_batch")
    ids["transformer_batch + argmax_batch"] = gpu.argmax_batch(states[:3]).tolist()
    for n in (3, 33):
        ids[f"transformer_wide n={n}"] = gpu.transformer_wide(states[:n], np.arange(1, n + 1), [0] * n, w).tolist()
        row(states[n - 1].logits(), f"l2z_transformer_wide n={n}")
    ids["wide_run at temperature 0"] = gpu.wide_run(states[:3], [1, 2, 3], 0, w, 2, 0.0, 1.0, None).reshape(-1).tolist()
    got = gpu.step_mixed(states[:3], [[1, 2, 3, 4], [5], [6, 7]], 0, w)
    row(states[0].logits(), "l2z_step_mixed (a prompt chunk)")
    row(states[1].logits(), "l2z_step_mixed (a decode row)")
    ids["step_mixed"] = got.tolist()

    # ---- the verify family: every returned id; the scan's id is accepted as a guess, any other is cut
    full, cut = [1, want, want, want], [1, want, wrong, want]
    for fam, call in (("verify", lambda t: states[0].verify(t, 0, w)),
                      ("verify_sample at temperature 0", lambda t: states[0].verify_sample(t, 0, w, 0.0, 1.0, None))):
        nxt, acc = call(full)
        for i in range(4):
            row(states[0].verify_logits(i), f"l2z_{fam} row {i}")
        assert acc == 3 or nxt.tolist() != [want] * 4, f"{fam}: a guess equal to its own id was refused"
        ids[fam] = nxt.tolist()
        nxt, acc = call(cut)
        assert acc == 1 or nxt.tolist() != [want] * 4, f"{fam}: accepted {acc} of {cut}"
        ids[fam] += nxt.tolist()
    for fam, call in (("verify_batch", gpu.verify_batch), ("verify_wide", gpu.verify_wide)):
        nxts, acc = call(states[:3], [full, cut, [2]], 0, w)
        for r in range(9):
            row(states[0].verify_logits(r), f"l2z_{fam} row {r}")
        ids[fam] = np.concatenate(nxts).tolist()
        assert acc.tolist() == [3, 1, 0] or ids[fam] != [want] * 9, f"{fam}: accepted {acc.tolist()}"
    nxt, path, acc = states[0].verify_tree([1, want, wrong, want, wrong], [-1, 0, 0, 1, 1], 0, w)
    for i in range(5):
        row(states[0].verify_logits(i), f"l2z_verify_tree node {i}")
    ids["verify_tree"] = nxt.tolist()
    assert (path.tolist() == [0, 1, 3] and acc == 2) or nxt.tolist() != [want] * 5, f"verify_tree: walked {path.tolist()}"

    # ---- l2z_score: top-1 of every position; the log-prob where the row holds no NaN
    toks = np.array([1, V - 1, 5, 4099 % V, 5000 % V], np.int32)   # targets: a tied maximum, -inf columns, a plain one
    lp, top = states[0].score(toks, 0, w)
    ids["score top-1"] = top.tolist()
    if case in ("pinf_70_and_last", "neginf_segment", "neginf_wave"):
        with np.errstate(invalid="ignore"):
            z = lg.astype(np.float64)
            ref = z - (z.max() + np.log(np.exp(z - z.max()).sum()))
        bar = 2.0 * (LOGIT_ATOL + LOGIT_RTOL * float(np.abs(z[np.isfinite(z)]).max()))
        for p in range(4):
            r, g = float(ref[toks[p + 1]]), float(lp[p])
            print(f"score {case} x3={x3} position {p}: log-prob {g}, float64 {r}, bar {bar:.2e}")
            assert (np.isnan(r) and np.isnan(g)) or r == g or abs(r - g) <= bar, (p, g, r)
    close(states + [w, w4])

    off = {f: got for f, got in ids.items() if any(i != want for i in got)}
    print(f"V {V} {case} x3={x3}: the scan {want}; " + ("every family agrees" if not off else f"off: {off}"))
    assert not off and not bad_rows, (f"the scan returns {want}; these families returned something else: {off}; "
                                      f"{len(bad_rows)} logits rows off the planted pattern: {bad_rows[:6]}")


# ------------------------------------------------------------------------------------- all-NaN probabilities
@pytest.mark.gpu
@pytest.mark.parametrize("V", [1000, 8200])
def test_all_nan_probabilities_draw_the_host_samplers_token(gpu, ck, H, V):
    """A NaN, a +inf or nothing but -inf in the logits: softmax gives NaN everywhere, on the host and on the device.  The
    host's sample then falls through to n - 1 (coin < NaN never holds) and its sample_top_p to the argmax of the
    probabilities, 0."""
    rows = {"one_nan": np.zeros(V, np.float32), "one_pinf": np.zeros(V, np.float32), "all_neginf": np.full(V, -INF, np.float32)}
    rows["one_nan"][5] = NAN
    rows["one_pinf"][70] = INF
    cfg = hook_cfg(ck, V)
    states = [gpu.RunState(cfg) for _ in range(3)]
    coins = [0.0, 0.5, BELOW_ONE]
    wrong = []
    for name, x in rows.items():
        for s in states:
            s.write_logits(x)
        for temp in (0.5, 1.0):
            probs = states[0].probs(temp)
            for top_p in (0.0, 0.9, 1.0):
                want = [host_token(H, probs, top_p, c) for c in coins]
                assert want == ([0] * 3 if top_p == 0.9 else [V - 1] * 3)
                got = gpu.sample_batch(states, temp, top_p, coins).tolist()
                print(f"V {V} {name} temperature {temp} top_p {top_p}: drew {got}, the host {want}")
                if got != want:
                    wrong.append((name, temp, top_p, got, want))
        for s in states:
            assert np.array_equal(bits(s.logits()), bits(x))
    close(states)
    assert not wrong, f"(row, temperature, top_p, drawn, the host's): {wrong}"


@pytest.mark.gpu
def test_all_nan_probabilities_through_the_model_fed_samplers(gpu, ck, H):
    """l2z_wide_run, l2z_verify_sample, l2z_step_mixed and l2z_sample_run share sample_row with l2z_sample_batch: on the
    NaN-at-5 checkpoint at temperature 1, top_p 1 each draws what the host sampler draws."""
    V = 1024
    v = planted(V, "nan5_max37")
    cfg, w = make_model(gpu, ck, V, v, 2)
    states = [gpu.RunState(cfg) for _ in range(3)]
    states[0].transformer(1, 0, w)
    check_pattern(states[0].logits(), v, "l2z_transformer")
    want = host_token(H, states[0].probs(1.0), 1.0, 0.5)
    assert want == V - 1
    ids = {}
    ids["wide_run"] = gpu.wide_run(states, [1, 2, 3], 0, w, 2, 1.0, 1.0, 0.5).reshape(-1).tolist()
    nxt, acc = states[0].verify_sample([1, want, 7], 0, w, 1.0, 1.0, [0.5, 0.5, 0.5])
    assert acc == 1 or nxt.tolist() != [want] * 3
    ids["verify_sample"] = nxt.tolist()
    ids["step_mixed"] = gpu.step_mixed(states, [[1, 2, 3], [4], [5, 6]], 0, w, 1.0, 1.0, 0.5).tolist()
    states[0].greedy_begin([])
    ids["sample_run"] = states[0].sample_run(w, 2, 1.0, 1.0, [0.5, 0.5]).tolist()
    close(states + [w])
    off = {f: got for f, got in ids.items() if any(i != want for i in got)}
    print(f"all-NaN probabilities, the host draws {want}: " + ("every family agrees" if not off else f"off: {off}"))
    assert not off, f"the host sampler draws {want}; these families drew {off}"
