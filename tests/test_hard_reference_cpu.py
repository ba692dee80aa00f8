"""The hard checkpoints' reference (tests/hard_models.py) checked without a GPU, so that tests/test_gpu_hard_parity.py is not
vacuous: the float64 logits are finite and agree with the oracle inside the bar, every kind of blob puts the attention in
the regime it is named after -- measured in float64 at positions >= 128, every layer and head --, the per-row bar leaves at
most 5 % of a case's rows out of the token comparison, and the bar is the same from run to run.

The regimes' bounds: f32 expf(-x) is exactly 0 from x = 104 on (2^-150 = exp(-103.97)), and exp(-88) is the smallest
NORMAL float32, so a spread inside (20, 88) is a peaked softmax whose every term is still a normal number and a spread
above 104 is one in which some term underflows to 0 whatever the rounding.
"""
import numpy as np
import pytest

import hard_models as hm

FROM = 128   # the regimes are asserted from this position on: the contexts the segment and split forms cut into parts


@pytest.fixture(scope="module", params=hm.CASES, ids=hm.CASE_IDS)
def ref(request, ck, orc):
    return hm.reference(ck, orc, *request.param)


def test_blob_edits_are_what_the_kinds_say(ck):
    cfg = hm.config(ck, "kvmul3")
    plain = ck.carve(cfg, ck.synth_blob(cfg, False, hm.SEED), False)
    ch = np.random.default_rng([hm.SEED, 77]).choice(cfg.dim, 4, replace=False)
    assert len(set(ch.tolist())) == 4
    rest = np.setdiff1d(np.arange(cfg.dim), ch)
    for kind, q_scale in (("flat", 0), ("peaked", 8), ("onehot", 32), ("outlier", 4)):
        w = ck.carve(cfg, hm.hard_blob(ck, cfg, hm.SEED, kind), False)
        assert np.array_equal(w["wq"], plain["wq"] * np.float32(q_scale)), kind
        for name in plain:
            if name == "wq":
                continue
            if kind == "outlier" and name in ("rms_att_weight", "rms_ffn_weight", "token_embedding_table"):
                k = 8 if name == "token_embedding_table" else 16
                assert np.array_equal(w[name][:, ch], plain[name][:, ch] * np.float32(k)), (kind, name)
                assert np.array_equal(w[name][:, rest], plain[name][:, rest]), (kind, name)
            else:
                assert np.array_equal(w[name], plain[name]), (kind, name)


def test_chain_and_shapes(ck, ref):
    cfg, L = ref.cfg, ref.cfg.seq_len
    assert ref.T.shape == (L,) and ref.T[0] == 1 and ref.T[1:].min() >= 2 and ref.T.max() < cfg.vocab_size
    assert ref.z64.shape == (L, cfg.vocab_size) and ref.z64.dtype == np.float64
    assert ref.D.shape == ref.bar.shape == ref.margin.shape == ref.top.shape == (L,)
    assert L > FROM + 16 and all(p < L for p in hm.EDGES)
    assert cfg.n_heads > cfg.n_kv_heads > 1   # grouped kv heads
    assert {"kvmul3": 48, "hs64h": 64, "hs128h": 128}[ref.shape] == cfg.head_size


def test_float64_logits_are_finite_and_the_oracle_is_inside_the_bar(ref):
    assert np.isfinite(ref.z64).all() and np.isfinite(ref.z_default).all()
    assert np.isfinite(ref.D).all() and (ref.D > 0).all()
    err = np.abs(ref.z_default.astype(np.float64) - ref.z64).max(axis=1)
    print(f"{ref.shape}-{ref.kind}: D {ref.D.min():.2e} .. {ref.D.max():.2e}; oracle (default reading) at most "
          f"{float((err / ref.bar).max()):.3f} of its bar; max |z64| {np.abs(ref.z64).max():.1f}")
    assert (err <= ref.D).all()          # the default reading is one of the twelve
    assert (err <= ref.bar).all()
    assert np.array_equal(ref.bar, hm.LOGIT_ATOL + 4 * ref.D)


def test_the_regime_holds_in_float64(ref):
    sp = ref.spread[:, :, FROM:].ravel()
    above = float((sp > hm.EXP_ZERO).mean())
    inside = float(((sp > 20) & (sp < 88)).mean())
    print(f"{ref.shape}-{ref.kind}: spreads at pos >= {FROM}: min {sp.min():.1f} median {np.median(sp):.1f} max {sp.max():.1f}; "
          f"share above {hm.EXP_ZERO:.0f}: {above:.2f}, inside (20, 88): {inside:.2f}")
    if ref.kind == "flat":
        assert (ref.spread == 0).all()       # every position, not only the deep ones
        assert ref.uniform.all()
    elif ref.kind == "peaked":
        assert ((sp > 20) & (sp < 88)).all()
    elif ref.kind == "onehot":
        assert above >= 0.90
    elif ref.kind == "outlier":
        assert above >= 0.40 and inside >= 0.20
    if ref.kind != "flat":
        assert not ref.uniform[:, :, 1:].any()


def test_at_most_5_percent_of_the_rows_fall_under_the_margin_rule(ref):
    under = int((ref.margin <= 2 * ref.bar).sum())
    print(f"{ref.shape}-{ref.kind}: {under} of {ref.margin.size} rows with a float64 top-2 margin <= 2 * bar")
    assert under <= 0.05 * ref.margin.size
    # where the margin exceeds twice the bar, every reading of the reference names the float64 model's token
    decided = ref.margin > 2 * ref.bar
    assert np.array_equal(np.argmax(ref.z_default, axis=1)[decided], ref.top[decided])


def test_the_spread_is_deterministic(ck, orc):
    """D from a second run of the twelve readings (the first 40 positions of the smallest shape's hardest case), bit for bit"""
    r = hm.reference(ck, orc, "kvmul3", "onehot")
    n = 40
    again = hm.spread_of(r.z64[:n], hm.readings(orc, r.cfg, r.blob, r.T[:n]))
    assert np.array_equal(again, r.D[:n])
    # ... and the oracle's mode is the default again
    m = orc.Model(r.cfg.as_i32(), r.blob, False)
    assert np.array_equal(m.transformer(1, 0), r.z_default[0])
    m.close()


def test_numpy_model_probe_is_off_by_default_and_changes_nothing(ck):
    from ref_numpy import NumpyModel
    cfg = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=128, seq_len=8)
    blob = ck.synth_blob(cfg, False, 3)
    seen = []
    a, b = NumpyModel(ck, cfg, blob, False), NumpyModel(ck, cfg, blob, False, probe=lambda *x: seen.append(x))
    assert a.probe is None
    for p, t in enumerate((1, 5, 9)):
        assert np.array_equal(a.transformer(t, p), b.transformer(t, p))
    assert [(l, h, p) for l, h, p, _, _ in seen] == [(l, h, p) for p in range(3) for l in range(2) for h in range(4)]
    for l, h, p, s, att in seen:
        assert att.shape == (p + 1,) and abs(att.sum() - 1) < 1e-12 and s >= 0 and (p > 0 or s == 0)
