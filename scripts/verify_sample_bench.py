"""l2z_verify_sample on the 7B shape (synthetic weights): what the sampled verdict adds to a verify pass, and what the sampled
speculative loop gains end to end over the plain sampled loop.  The method of scripts/verify_bench.py.

One process holds this build; with --parent-lib a CHILD process holds another build of the library (the parent commit's
libllama2_hip_test.so, through L2Z_LIB) and measures on request, so the two builds alternate inside one run on one GPU.

* call time, short (pos0 = 16) and long (pos0 = 2000) context, T = 1, 2, 4, 8, 16: l2z_verify_sample_time (this build) at
  -t 1 -p 0.9, -t 1 -p 1 and a peaked setting (-t 0.05: the distribution of "logits x 20") against the parent's l2z_verify_time
  at the same T.  The difference is the sampled verdict (sample_batch_kernel on T rows in place of the argmax launch).
  Device events over >= --seconds per reading after a warm-up of every shape; --rounds readings, best and worst given.
* end to end: binding.speculate_sample over 256 positions from a 32-token prompt at -t 1 -p 0.9 with a drafter that replays
  the K = 0 text, each guess made wrong with probability q, against the parent's route to sampled text through the same
  binding: per token l2z_transformer, l2z_probs_read and the host sampler.  The prompt's share is subtracted on both sides.
  Every (K, q) must emit the K = 0 ids (asserted).
The acceptance real text gives lookup_draft at -t 1 -p 0.9 is NOT measured here: no real checkpoint is in the tree, and
synthetic logits are near-uniform, so a natural guess is accepted with probability ~ 1 / nucleus size.

    python scripts/verify_sample_bench.py [--parent-lib PATH] [--out profiles/verify_sample_bench.md]
    rocprofv3 --kernel-trace --stats -d DIR -o p -- python scripts/verify_sample_bench.py --profile --T 8 --pos 2000
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TS = (1, 2, 4, 8, 16)
CONTEXTS = (16, 2000)
SETTINGS = (("-t 1 -p 0.9", 1.0, 0.9), ("-t 1 -p 1", 1.0, 1.0), ("-t 0.05 -p 0.9 (peaked)", 0.05, 0.9))
N_PROMPT, N_GEN = 32, 256
E2E_T, E2E_P, E2E_SEED = 1.0, 0.9, 1


def load():
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    return np, pkg.binding, pkg.checkpoint


def stream_of(np, cfg, n):
    return np.random.default_rng(7).integers(2, cfg.vocab_size, n).astype(np.int32)


def iters_for(ms, seconds):
    return max(8, int(seconds * 1e3 / ms) + 1)


def plain_sampled(np, B, s, w, prompt, coins):
    """the plain sampled loop (llama2_main.cpp's, through the binding): the prompt as one prefill, then per token
    l2z_transformer, l2z_probs_read and the host sampler.  Returns ms per generated token behind the first."""
    H = B.host_lib()
    fp = C.POINTER(C.c_float)
    H.l2zh_sample_top_p_coin.restype = C.c_size_t
    H.l2zh_sample_top_p_coin.argtypes = [fp, C.c_size_t, C.c_float, C.c_float, fp]
    s.prefill(np.array([1] + prompt[:-1], np.int32), 0, w)
    token, pos = prompt[-1], len(prompt)
    t0 = None
    for g in range(N_GEN):
        s.transformer(int(token), pos, w)
        p = s.probs(E2E_T)
        token = int(H.l2zh_sample_top_p_coin(p.ctypes.data_as(fp), p.size, C.c_float(E2E_P), C.c_float(float(coins[g])), None))
        pos += 1
        if t0 is None:
            t0 = time.perf_counter()
    return (time.perf_counter() - t0) * 1e3 / (N_GEN - 1)


def child():
    """The library L2Z_LIB names.  One line in, one line out (milliseconds): "verify T pos seconds", "plain"."""
    np, B, ck = load()
    cfg = ck.LLAMA2_7B
    w = B.Weights(cfg, None, False, seed=1)
    toks = stream_of(np, cfg, cfg.seq_len)
    s, at = B.RunState(cfg), -1
    print("ready", flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "verify":
            T, pos, seconds = int(cmd[1]), int(cmd[2]), float(cmd[3])
            if at != pos:
                s.prefill(toks[:pos], 0, w)
                at = pos
            ms = s.verify_time(toks[pos:pos + T], pos, w, 8)
            ms = s.verify_time(toks[pos:pos + T], pos, w, iters_for(ms, seconds))
        else:
            at = -1
            ms = plain_sampled(np, B, s, w, [int(t) for t in toks[:N_PROMPT]], B.coin_stream(E2E_SEED, N_GEN))
        print(f"{ms:.5f}", flush=True)
    s.close(); w.close()


def profile(a):
    np, B, ck = load()
    cfg = ck.LLAMA2_7B
    w = B.Weights(cfg, None, False, seed=1)
    toks = stream_of(np, cfg, cfg.seq_len)
    s = B.RunState(cfg)
    if a.pos:
        s.prefill(toks[:a.pos], 0, w)
    for _, t, p in SETTINGS:
        for _ in range(4):
            s.verify_sample(toks[a.pos:a.pos + a.T], a.pos, w, t, p, B.coin_stream(3, a.T))
    s.close(); w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_sample_bench.md"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--seconds", type=float, default=1.0, help="device time per reading of a call time")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--profile", action="store_true",
                    help="nothing but 4 calls of T rows at --pos per setting (the program of a rocprofv3 --kernel-trace run)")
    ap.add_argument("--T", type=int, default=8)
    ap.add_argument("--pos", type=int, default=2000)
    a = ap.parse_args()
    if a.child:
        return child()
    if a.profile:
        return profile(a)
    kid = None
    if a.parent_lib:   # started before this process touches the GPU
        kid = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], stdin=subprocess.PIPE,
                               stdout=subprocess.PIPE, text=True, env=dict(os.environ, L2Z_LIB=os.path.abspath(a.parent_lib)))
        assert kid.stdout.readline().strip() == "ready", "the child with the parent build did not start"

    def parent(cmd):
        if kid is None:
            return float("nan")
        kid.stdin.write(cmd + "\n"); kid.stdin.flush()
        return float(kid.stdout.readline())

    np, B, ck = load()
    cfg = ck.LLAMA2_7B
    w, s = B.Weights(cfg, None, False, seed=1), B.RunState(cfg)
    name = B.device_info(0)[0]
    toks = stream_of(np, cfg, cfg.seq_len)
    coins16 = B.coin_stream(3, 16)
    fmt = lambda x: "not measured" if min(x) != min(x) else f"{min(x):.3f} .. {max(x):.3f}"
    out = [f"# l2z_verify_sample, Llama-2-7B shape, synthetic weights (scripts/verify_sample_bench.py)\n\nDevice: {name}.  "
           "\"parent\": the parent commit's build in a second process"
           + ("" if kid else " -- NOT MEASURED (no --parent-lib)") + f", alternating with this build; {a.rounds} readings per figure "
           f"after a warm-up of every shape, best .. worst.  Call times: device events over >= {a.seconds:g} s of passes back to "
           "back (l2z_verify_sample_time / the parent's l2z_verify_time), the verdict and its copy included.  \"verdict\": best "
           "minus the parent's best -- sample_batch_kernel on T rows in place of the argmax launch; its prior is the table of "
           "DESIGN.md 4.8 for the same kernel (0.06 - 0.27 ms per launch at vocab 32000, the slowest row deciding).\n"]

    # ---- call times
    step = {}
    for pos in CONTEXTS:
        s.prefill(toks[:pos], 0, w)
        for T in TS:   # warm-up of every shape
            for _, t, p in SETTINGS:
                s.verify_sample_time(toks[pos:pos + T], pos, w, t, p, coins16[:T], 4)
            parent(f"verify {T} {pos} 0.05")
        out.append(f"\n## Call time at pos0 = {pos}\n\n| T | parent l2z_verify (ms) | "
                   + " | ".join(f"{n} (ms) | verdict (ms)" for n, _, _ in SETTINGS) + " |\n|---:|---:|" + "---:|---:|" * len(SETTINGS) + "\n")
        for T in TS:
            rows = toks[pos:pos + T]
            b = []
            v = [[] for _ in SETTINGS]
            ms0 = s.verify_sample_time(rows, pos, w, 1.0, 0.9, coins16[:T], 8)
            for _ in range(a.rounds):
                b.append(parent(f"verify {T} {pos} {a.seconds}"))
                for i, (_, t, p) in enumerate(SETTINGS):
                    v[i].append(s.verify_sample_time(rows, pos, w, t, p, coins16[:T], iters_for(ms0, a.seconds)))
            step[(pos, T)] = min(v[0])
            cells = " | ".join(f"{fmt(x)} | " + ("" if min(b) != min(b) else f"{min(x) - min(b):+.3f}") for x in v)
            out.append(f"| {T} | {fmt(b)} | {cells} |\n")
            print(f"pos0 {pos} T {T}: parent verify {fmt(b)} | " + " | ".join(fmt(x) for x in v), flush=True)

    # ---- end to end
    prompt = [int(t) for t in toks[:N_PROMPT]]
    steps = N_PROMPT + N_GEN
    coins = B.coin_stream(E2E_SEED, N_GEN)

    def timed(k, drafter, n_steps=steps):
        st = B.RunState(cfg)
        t0 = time.perf_counter()
        got, stats = B.speculate_sample(st, w, prompt, n_steps, k, E2E_T, E2E_P, coins, drafter)
        dt = time.perf_counter() - t0
        st.close()
        return got, stats, dt

    timed(0, None, N_PROMPT + 1)
    t_prompt = min(timed(0, None, N_PROMPT + 1)[2] for _ in range(3))
    base, st0, dt0 = timed(0, None)
    full = np.concatenate([[1], base]).astype(np.int32)
    n_gen = len(base) - N_PROMPT - 1   # positions decoded by verify_sample calls
    plain = [parent("plain") for _ in range(a.rounds)]
    plain_ms = min(plain)
    out.append(f"\n## End to end: {N_GEN} positions behind a {N_PROMPT}-token prompt, -t {E2E_T:g} -p {E2E_P:g}\n\nParent's plain sampled "
               "loop (l2z_transformer, l2z_probs_read, host sampler per token; wall clock behind the first generated token): "
               + ("not measured" if plain_ms != plain_ms else f"{fmt(plain)} ms / token = {1e3 / plain_ms:.1f} tokens/s at best")
               + f".  speculate_sample: wall clock of the call minus the prompt's share ({t_prompt * 1e3:.1f} ms: a run of "
               f"{N_PROMPT + 1} positions), over the {n_gen} positions its calls decode"
               + (" (the run ended early at a BOS)" if 1 in base.tolist() else "")
               + f", best .. worst of {max(2, a.rounds // 2)}.  Drafter: the K = 0 text replayed, each guess replaced by a wrong id with "
               "probability q.  Every row emitted the K = 0 ids (asserted).\n\n"
               "| K | q | tokens / call | guesses offered | accepted | ms / token | tokens/s | x plain |\n|---:|---:|---:|---:|---:|---:|---:|---:|\n")
    rows_e2e = [(0, 0.0, None)] + [(k, q, "replay") for k in (3, 7, 15) for q in (0.0, 0.25, 0.5, 0.75, 1.0)]
    e2e = {}
    for k, q, kind in rows_e2e:
        runs = []
        for _ in range(max(2, a.rounds // 2)):
            rng = np.random.default_rng(int(q * 100) + k)

            def drafter(hist, kk):
                g = full[len(hist):len(hist) + kk].copy()
                bad = rng.random(len(g)) < q
                g[bad] = (g[bad] - 2 + 1) % (cfg.vocab_size - 2) + 2
                return g

            got, stats, dt = timed(k, drafter if kind else None)
            assert got.tolist() == base.tolist(), "the ids depend on the drafter"
            runs.append((dt - t_prompt) * 1e3 / max(n_gen, 1))
        e2e[(k, q)] = (min(runs), max(runs))
        rel = "" if plain_ms != plain_ms else f"{plain_ms / min(runs):.2f}"
        out.append(f"| {k} | {q:g} | {stats['emitted'] / max(stats['calls'], 1):.2f} | {stats['offered']} | {stats['accepted']} | "
                   f"{fmt(runs)} | {1e3 / min(runs):.1f} | {rel} |\n")
        print(f"K {k} q {q}: {stats} {fmt(runs)} ms/token", flush=True)
    if plain_ms == plain_ms:
        out.append("\nBreak-even (tokens per call at which the loop equals the plain sampled loop) = call time at -t 1 -p 0.9 / plain "
                   "ms per token, short context: " + ", ".join(f"T = {T}: {step[(CONTEXTS[0], T)] / plain_ms:.2f}" for T in TS) + ".\n")
        for k in (7, 15):
            lo, hi = e2e[(k, 0.0)]
            gain, spreads = plain_ms - lo, (hi - lo) + (max(plain) - plain_ms)
            verdict = "faster than the plain loop by more than the two spreads together" if gain > spreads else \
                "NOT faster than the plain loop by more than the two spreads together"
            out.append(f"\nK = {k}, q = 0: {lo:.3f} ms / token against {plain_ms:.3f} plain: a gain of {gain:.3f} ms, the two spreads "
                       f"together {spreads:.3f} ms -- {verdict}.\n")
    out.append("\nNot measured: the acceptance real text gives lookup_draft at -t 1 -p 0.9 (no real checkpoint is in the tree; on "
               "near-uniform synthetic logits a natural guess is accepted with probability ~ 1 / nucleus size).\n")
    if kid:
        kid.stdin.write("quit\n"); kid.stdin.flush(); kid.wait(timeout=60)
    s.close(); w.close()
    with open(a.out, "w") as f:
        f.write("".join(out))


if __name__ == "__main__":
    main()
