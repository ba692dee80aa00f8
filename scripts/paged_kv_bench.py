#!/usr/bin/env python3
"""What a page table costs the wide family: l2z_transformer_wide and l2z_verify_wide on PAGED runstates (a KV page pool,
include/llama2_hip_test.h) against the same calls on contiguous runstates, on this build, alternating in one process.

7B dims with seq_len 1024 (so that 128 contiguous caches of 1 GB fit beside the weights and the pool), n = 64 and 128,
positions below 32 and around 500: one transformer_wide step; and one verify_wide call of 32 sequences x 4 rows.  A round is
one call by a host clock, ending in a synchronize of every runstate; best of --rounds, all readings listed.  The paged
sequences get their lower pages by l2z_runstate_fork from the contiguous ones (the rows' contents do not change the work).
Then the case no contiguous form can run: 128 paged sequences at the model's own seq_len of 2048, and the pool bytes in use
against the 275 GB that 128 contiguous runstates would reserve.  Synthetic weights.

  python scripts/paged_kv_bench.py [--rounds 6] [--md profiles/paged_kv_bench.md]
  python scripts/paged_kv_bench.py --profile-step paged|contiguous   # three n = 128 steps at pos ~500 for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def positions(n, deep, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    return rng.integers(484, 516, size=n).astype(np.int32) if deep else rng.integers(0, 32, size=n).astype(np.int32)


def best_of(rounds, calls, sync):
    """the calls alternate; per call the list of wall times in ms"""
    out = [[] for _ in calls]
    for f in calls:   # warm-up: allocations, code objects, page attachment
        f()
        sync()
    for _ in range(rounds):
        for f, t in zip(calls, out):
            t0 = time.perf_counter()
            f()
            sync()
            t.append(round((time.perf_counter() - t0) * 1e3, 3))
    return out


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--md", default=None)
    ap.add_argument("--profile-step", default=None, choices=["paged", "contiguous"])
    a = ap.parse_args()
    pkg = ge.load_package()
    B, ck = pkg.binding, pkg.checkpoint
    seven = ck.LLAMA2_7B

    def cfg_of(seq_len):
        return ck.Config(seven.dim, seven.hidden_dim, seven.n_layers, seven.n_heads, seven.n_kv_heads, seven.vocab_size, seq_len)
    N, PAGE = 128, B.KV_PAGE
    rows, lines = [], []

    cfg = cfg_of(1024)
    w = B.Weights(cfg, None, False, seed=2024)
    pool = B.KvPool(cfg, N * 9)
    page_bytes = pool.info()["page_bytes"]
    cont = [B.RunState(cfg) for _ in range(N)]
    paged = [B.RunState(cfg, pool=pool) for _ in range(N)]

    def sync_of(ss):
        def sync():
            for s in ss:
                s.synchronize()
        return sync

    if a.profile_step:
        pos, tok = positions(N, True, N), (7 + np.arange(N)).astype(np.int32)
        ss = paged if a.profile_step == "paged" else cont
        if a.profile_step == "paged":
            for s, c, p in zip(paged, cont, pos):
                B.runstate_fork(s, c, int(p))
        for _ in range(3):
            B.transformer_wide(ss, tok, pos, w)
        return

    for deep in (False, True):
        for n in (64, N):
            pos, tok = positions(n, deep, n), (7 + np.arange(n)).astype(np.int32)
            for s, c, p in zip(paged[:n], cont[:n], pos):
                B.runstate_fork(s, c, int(p))   # pages for every position below p
            c_ms, p_ms = best_of(a.rounds, [lambda: B.transformer_wide(cont[:n], tok, pos, w, want_next=False),
                                            lambda: B.transformer_wide(paged[:n], tok, pos, w, want_next=False)],
                                 sync_of(cont[:n] + paged[:n]))
            rows.append({"call": "transformer_wide", "n": n, "rows": n, "context": "pos ~500" if deep else "pos < 32",
                         "pos_min": int(pos.min()), "pos_max": int(pos.max()), "contiguous_ms": min(c_ms), "paged_ms": min(p_ms),
                         "contiguous_ms_all": c_ms, "paged_ms_all": p_ms})
            print(json.dumps(rows[-1]), flush=True)
        # verify_wide: 32 sequences x 4 rows
        n = 32
        pos = positions(n, deep, 3 * n)
        lists = [np.array([5 + j, 6, 7, 8], np.int32) for j in range(n)]
        for s, c, p in zip(paged[:n], cont[:n], pos):
            B.runstate_fork(s, c, int(p))
        c_ms, p_ms = best_of(a.rounds, [lambda: B.verify_wide(cont[:n], lists, pos, w),
                                        lambda: B.verify_wide(paged[:n], lists, pos, w)], sync_of(cont[:n] + paged[:n]))
        rows.append({"call": "verify_wide", "n": n, "rows": 4 * n, "context": "pos ~500" if deep else "pos < 32",
                     "pos_min": int(pos.min()), "pos_max": int(pos.max()), "contiguous_ms": min(c_ms), "paged_ms": min(p_ms),
                     "contiguous_ms_all": c_ms, "paged_ms_all": p_ms})
        print(json.dumps(rows[-1]), flush=True)
    for s in cont + paged:
        s.close()
    pool.close()
    w.close()

    # ---- the model's own seq_len: 128 sequences, paged only ----
    cfg = cfg_of(2048)
    contiguous_bytes = N * 2 * cfg.n_layers * cfg.seq_len * (cfg.dim // cfg.n_heads * cfg.n_kv_heads) * 4
    w = B.Weights(cfg, None, False, seed=2024)
    pool = B.KvPool(cfg, N * 9)
    paged = [B.RunState(cfg, pool=pool) for _ in range(N)]
    tok = (7 + np.arange(N)).astype(np.int32)
    long_rows = []
    for deep in (False, True):
        pos = positions(N, deep, N)
        if deep:   # the pages below: one wide step per page (what they hold does not change the work)
            for p0 in range(PAGE, 512, PAGE):
                B.transformer_wide(paged, tok, np.full(N, p0, np.int32), w, want_next=False)
        (p_ms,) = best_of(a.rounds, [lambda: B.transformer_wide(paged, tok, pos, w, want_next=False)], sync_of(paged))
        info = pool.info()
        used = (info["n_pages"] - info["n_free"]) * info["page_bytes"]
        long_rows.append({"call": "transformer_wide", "seq_len": 2048, "n": N, "context": "pos ~500" if deep else "pos < 32",
                          "paged_ms": min(p_ms), "paged_ms_all": p_ms, "pool_bytes_in_use": used,
                          "contiguous_bytes": contiguous_bytes})
        print(json.dumps(long_rows[-1]), flush=True)
    for s in paged:
        s.close()
    pool.close()
    w.close()

    lines.append("| call | context | sequences (rows) | contiguous ms | paged ms | paged / contiguous | contiguous readings | paged readings |")
    lines.append("|---|---|---:|---:|---:|---:|---|---|")
    for r in rows:
        lines.append(f"| {r['call']} | {r['context']} ({r['pos_min']}-{r['pos_max']}) | {r['n']} ({r['rows']}) | "
                     f"{r['contiguous_ms']:.3f} | {r['paged_ms']:.3f} | {r['paged_ms'] / r['contiguous_ms']:.3f} | "
                     f"{', '.join(f'{x:.3f}' for x in r['contiguous_ms_all'])} | {', '.join(f'{x:.3f}' for x in r['paged_ms_all'])} |")
    lines.append("")
    lines.append("| seq_len 2048, 128 paged sequences | paged ms / step | readings | pool in use | contiguous caches would reserve |")
    lines.append("|---|---:|---|---:|---:|")
    for r in long_rows:
        lines.append(f"| {r['context']} | {r['paged_ms']:.3f} | {', '.join(f'{x:.3f}' for x in r['paged_ms_all'])} | "
                     f"{r['pool_bytes_in_use'] / 1e9:.1f} GB | {r['contiguous_bytes'] / 1e9:.0f} GB |")
    text = "\n".join(lines)
    print("\n" + text)
    if a.md:
        with open(a.md, "w") as f:
            f.write(f"# Paged KV cache: the wide family on a page pool against contiguous caches\n\n"
                    f"`python scripts/paged_kv_bench.py --rounds {a.rounds}` on {B.device_info(0)[0]}; llama2-7b dims, synthetic "
                    f"weights; a page is {page_bytes / 1e6:.0f} MB.  Wall ms per call, best of {a.rounds}, the two forms "
                    f"alternating in one process.\n\n" + text + "\n")


if __name__ == "__main__":
    main()
