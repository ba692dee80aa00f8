"""l2z_verify on the 7B shape (synthetic weights): what a pass over T positions of one sequence costs against the two routes
the parent commit has to the same verdict, and what the speculative greedy loop gains end to end.

One process holds this build; with --parent-lib a CHILD process holds another build of the library (the parent commit's
libllama2_hip_test.so, through L2Z_LIB) and measures on request, so the two builds alternate inside one run on one GPU.

* step times, short (pos0 = 16) and long (pos0 = 2000) context, T = 1, 2, 4, 8, 16: l2z_verify_time (this build) against the
  parent's l2z_batch_time with n = T on T forks of the prompt (the same products; T caches read) and, at the long context,
  the parent's l2z_score of T tokens at pos0 (wall clock of the synchronous call).  Device events over >= --seconds per
  reading after a warm-up of every shape; --rounds readings, best and worst given.
* end to end: binding.speculate_greedy over 256 positions from a 32-token prompt with a drafter that replays the model's own
  continuation, each guess corrupted with probability q, against the parent's l2z_greedy_run over the same positions.  The
  prompt's share (a run of prompt + 1 positions) is subtracted on both sides.
* lookup_draft on the synthetic model's own greedy output -- a curiosity: synthetic weights write no natural text, so the
  acceptance a real prompt gives the drafter is NOT measured here -- and its host time per call at a 2000-token history.

    python scripts/verify_bench.py [--parent-lib PATH] [--out profiles/verify_bench.md]
    rocprofv3 --kernel-trace --stats -d DIR -o p -- python scripts/verify_bench.py --profile verify --T 8 --pos 2000
    (--profile batch: the same rows through l2z_transformer_batch, the parent's route, for its attention kernel's time)
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TS = (1, 2, 4, 8, 16)
CONTEXTS = (16, 2000)
N_PROMPT, N_GEN = 32, 256


def load():
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    return np, pkg.binding, pkg.checkpoint


def stream_of(np, cfg, n):
    return np.random.default_rng(7).integers(2, cfg.vocab_size, n).astype(np.int32)


class Forks:
    """T runstates holding one prompt of `pos` positions (prefill once, l2z_runstate_fork)"""

    def __init__(self, B, cfg, w, toks):
        self.B, self.cfg, self.w, self.toks, self.ss, self.pos = B, cfg, w, toks, [B.RunState(cfg)], -1

    def at(self, pos, T):
        B = self.B
        while len(self.ss) < T:
            self.ss.append(B.RunState(self.cfg))
        if pos != self.pos:
            self.ss[0].prefill(self.toks[:pos], 0, self.w)
            self.pos, self.forked = pos, 1
        for i in range(self.forked, T):
            B.runstate_fork(self.ss[i], self.ss[0], pos)
        self.forked = max(self.forked, T)
        return self.ss[:T]


def iters_for(ms, seconds):
    return max(8, int(seconds * 1e3 / ms) + 1)


def child():
    """The library L2Z_LIB names.  One line in, one line out (milliseconds): "batch T pos seconds", "score T pos",
    "greedy" (l2z_greedy_run over N_GEN positions behind the N_PROMPT-token prompt)."""
    np, B, ck = load()
    cfg = ck.LLAMA2_7B
    w = B.Weights(cfg, None, False, seed=1)
    toks = stream_of(np, cfg, cfg.seq_len)
    forks = Forks(B, cfg, w, toks)
    print("ready", flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "batch":
            T, pos, seconds = int(cmd[1]), int(cmd[2]), float(cmd[3])
            ss = forks.at(pos, T)
            rows, ps = [int(toks[pos])] * T, [pos] * T
            ms = B.batch_time(ss, rows, ps, w, 8)
            ms = B.batch_time(ss, rows, ps, w, iters_for(ms, seconds))
        elif cmd[0] == "score":
            T, pos = int(cmd[1]), int(cmd[2])
            s = forks.at(pos, 1)[0]
            t0 = time.perf_counter()
            s.score(toks[pos:pos + T], pos, w)
            ms = (time.perf_counter() - t0) * 1e3
        else:
            s = forks.at(0, 1)[0] if forks.pos == 0 else forks.ss[0]
            forks.pos = -1
            prompt = toks[:N_PROMPT]
            s.greedy_begin(prompt)
            s.greedy_run(w, N_PROMPT + 1)
            t0 = time.perf_counter()
            got = s.greedy_run(w, N_GEN - 1)
            ms = (time.perf_counter() - t0) * 1e3 / max(len(got), 1)
        print(f"{ms:.5f}", flush=True)
    w.close()


def profile(a):
    np, B, ck = load()
    cfg = ck.LLAMA2_7B
    w = B.Weights(cfg, None, False, seed=1)
    toks = stream_of(np, cfg, cfg.seq_len)
    if a.profile == "verify":
        s = B.RunState(cfg)
        if a.pos:
            s.prefill(toks[:a.pos], 0, w)
        for _ in range(4):
            s.verify(toks[a.pos:a.pos + a.T], a.pos, w)
    else:
        ss = Forks(B, cfg, w, toks).at(a.pos, a.T)
        for _ in range(4):
            B.transformer_batch(ss, [int(toks[a.pos])] * a.T, [a.pos] * a.T, w)
        ss[0].synchronize()
    w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_bench.md"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--seconds", type=float, default=1.0, help="device time per reading of a step time")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--profile", choices=("verify", "batch"), default=None,
                    help="nothing but 4 calls of T rows at --pos (the program of a rocprofv3 --kernel-trace run)")
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
    out = [f"# l2z_verify, Llama-2-7B shape, synthetic weights (scripts/verify_bench.py)\n\nDevice: {name}.  \"parent\": the "
           "parent commit's build in a second process"
           + ("" if kid else " -- NOT MEASURED (no --parent-lib)") + f", alternating with this build; {a.rounds} readings per figure "
           f"after a warm-up of every shape, best .. worst.  Step times: device events over >= {a.seconds:g} s of passes back to "
           "back (l2z_verify_time / l2z_batch_time); l2z_score: wall clock of the synchronous call.\n"]

    # ---- step times
    step = {}
    for pos in CONTEXTS:
        s.prefill(toks[:pos], 0, w)
        for T in TS:   # warm-up of every shape
            s.verify_time(toks[pos:pos + T], pos, w, 4)
            parent(f"batch {T} {pos} 0.05")
            if pos > 100:
                parent(f"score {T} {pos}")
        out.append(f"\n## Step time at pos0 = {pos}\n\n| T | l2z_verify (ms) | parent l2z_transformer_batch, n = T (ms) | parent "
                   "l2z_score of T tokens (ms) | verify / batch |\n|---:|---:|---:|---:|---:|\n")
        for T in TS:
            v, b, sc = [], [], []
            rows = toks[pos:pos + T]
            ms0 = s.verify_time(rows, pos, w, 8)
            for _ in range(a.rounds):
                b.append(parent(f"batch {T} {pos} {a.seconds}"))
                v.append(s.verify_time(rows, pos, w, iters_for(ms0, a.seconds)))
                sc.append(parent(f"score {T} {pos}") if pos > 100 else float("nan"))
            step[(pos, T)] = (min(v), max(v), min(b), max(b), min(sc), max(sc))
            fmt = lambda x: "not measured" if min(x) != min(x) else f"{min(x):.3f} .. {max(x):.3f}"
            ratio = "" if min(b) != min(b) else f"{min(v) / min(b):.3f}"
            out.append(f"| {T} | {fmt(v)} | {fmt(b)} | {fmt(sc)} | {ratio} |\n")
            print(f"pos0 {pos} T {T}: verify {fmt(v)} | parent batch {fmt(b)} | parent score {fmt(sc)}", flush=True)

    # ---- end to end
    prompt = [int(t) for t in toks[:N_PROMPT]]
    steps = N_PROMPT + N_GEN

    def timed(k, drafter, n_steps=steps):
        st = B.RunState(cfg)
        t0 = time.perf_counter()
        got, stats = B.speculate_greedy(st, w, prompt, n_steps, k, drafter)
        dt = time.perf_counter() - t0
        st.close()
        return got, stats, dt

    timed(0, None, N_PROMPT + 1)
    t_prompt = min(timed(0, None, N_PROMPT + 1)[2] for _ in range(3))
    base, st0, dt0 = timed(0, None)
    full = np.concatenate([[1], base]).astype(np.int32)
    n_gen = len(base) - N_PROMPT - 1   # positions decoded by verify calls
    plain = [parent("greedy") for _ in range(3)]
    plain_ms = min(plain)
    out.append(f"\n## End to end: {N_GEN} positions behind a {N_PROMPT}-token prompt\n\nParent l2z_greedy_run: "
               + ("not measured" if plain_ms != plain_ms else f"{plain_ms:.3f} ms / token = {1e3 / plain_ms:.1f} tokens/s "
                  f"(readings {', '.join(f'{x:.3f}' for x in plain)})")
               + f".  speculate_greedy: wall clock of the call minus the prompt's share ({t_prompt * 1e3:.1f} ms: a run of "
               f"{N_PROMPT + 1} positions), over the {n_gen} positions its verify calls decode"
               + (" (the run ended early at a BOS)" if 1 in base.tolist() else "")
               + ".  Drafter: the model's own continuation replayed, each guess replaced by a wrong id with probability q.\n\n"
               "| K | q | tokens / call | guesses offered | accepted | ms / token | tokens/s | x plain |\n|---:|---:|---:|---:|---:|---:|---:|---:|\n")
    rows_e2e = [(0, 0.0, None)] + [(k, q, "replay") for k in (3, 7, 15) for q in (0.0, 0.25, 0.5, 0.75, 1.0)]
    for k, q, kind in rows_e2e:
        rng = np.random.default_rng(int(q * 100) + k)

        def drafter(hist, kk):
            g = full[len(hist):len(hist) + kk].copy()
            bad = rng.random(len(g)) < q
            g[bad] = (g[bad] - 2 + 1) % (cfg.vocab_size - 2) + 2
            return g

        got, stats, dt = min((timed(k, drafter if kind else None) for _ in range(2)), key=lambda r: r[2])
        assert got.tolist() == base.tolist(), "the ids depend on the drafter"
        ms = (dt - t_prompt) * 1e3 / max(n_gen, 1)
        rel = "" if plain_ms != plain_ms else f"{plain_ms / ms:.2f}"
        out.append(f"| {k} | {q:g} | {stats['emitted'] / max(stats['calls'], 1):.2f} | {stats['offered']} | {stats['accepted']} | "
                   f"{ms:.3f} | {1e3 / ms:.1f} | {rel} |\n")
        print(f"K {k} q {q}: {stats} {ms:.3f} ms/token", flush=True)
    if plain_ms == plain_ms:
        out.append("\nBreak-even (tokens per call at which the loop equals plain decoding) = verify step time / plain step time, "
                   "short context: " + ", ".join(f"T = {T}: {step[(CONTEXTS[0], T)][0] / plain_ms:.2f}" for T in TS) + ".\n")

    # ---- the drafter itself
    got, stats, dt = timed(7, None)
    assert got.tolist() == base.tolist()
    hist = np.random.default_rng(3).integers(2, cfg.vocab_size, 2000).astype(np.int32)
    hist[-3:] = hist[5:8]   # one 3-gram hit far back: the whole history is scanned once
    B.lookup_draft(hist, 7)
    t0 = time.perf_counter()
    for _ in range(2000):
        B.lookup_draft(hist, 7)
    us_hit = (time.perf_counter() - t0) / 2000 * 1e6
    hist2 = np.arange(2, 2002, dtype=np.int32)   # no repeat: three full scans
    t0 = time.perf_counter()
    for _ in range(2000):
        B.lookup_draft(hist2, 7)
    us_miss = (time.perf_counter() - t0) / 2000 * 1e6
    out.append(f"\n## lookup_draft\n\nA curiosity, not a claim: on the synthetic model's OWN greedy output (which is no natural text "
               f"and may cycle) K = 7 with lookup_draft offered {stats['offered']} guesses in {stats['calls']} calls, {stats['accepted']} "
               f"accepted, {stats['emitted'] / max(stats['calls'], 1):.2f} tokens / call, {(dt - t_prompt) * 1e3 / max(n_gen, 1):.3f} ms / token.  "
               "The acceptance a real prompt gives the drafter is not measured here (no real checkpoint or text in the tree).\n\n"
               f"Host time per call at a 2000-token history, through the Python binding (ctypes call included): {us_hit:.1f} us with "
               f"one 3-gram hit at the far end, {us_miss:.1f} us without any repeat (three full scans).\n")
    if kid:
        kid.stdin.write("quit\n"); kid.stdin.flush(); kid.wait(timeout=60)
    s.close(); w.close()
    with open(a.out, "w") as f:
        f.write("".join(out))


if __name__ == "__main__":
    main()
