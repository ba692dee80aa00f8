"""The decode path's speed figures of ONE build of the library (L2Z_LIB names it), as one JSON line: l2z_time_kind of every
decode kind at the 7B shape (pos 0, 255, 2047) and at stories110M and stories15M (pos 0, 255), in us per launch, and the whole-token greedy
rate at the three shapes; and the same per-kind figures on int8 group-quantized weights at the 7B widths (one layer).  To compare two builds, alternate processes of this script (parent, head, a second copy of the
parent for the A/A spread) in one session and compare per round: profiles/decode_kernels_refactor.md.

usage: L2Z_LIB=/path/to/libllama2_hip_test.so python scripts/decode_speed.py >> figures.jsonl"""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, __graft_entry__ as ge
pkg = ge.load_package(); B, ck = pkg.binding, pkg.checkpoint
shapes = {n: (c, sh) for n, c, sh in ck.iter_configs()}
out = {"lib": os.environ.get("L2Z_LIB", "")}
for wl, positions, steps in (("llama2-7b", (0, 255, 2047), 150), ("stories110M", (0, 255), 600), ("stories15M", (0, 255), 250)):
    cfg, shared = shapes[wl]
    w, s = B.Weights(cfg, None, shared, seed=2024), B.RunState(cfg)
    for pos in positions:
        for kind in ("qkv", "attn", "wo", "ffn13", "ffn2", "cls", "argmax"):
            s.time_kind(kind, pos, w, reps=4)  # warm-up
            us = [s.time_kind(kind, pos, w, reps=16)[0] * 1e3 for _ in range(5)]
            out[f"{wl} pos {pos} {kind} us"] = float(np.median(us))
    rates = []
    for r in range(4):  # the first run captures the graphs
        s.greedy_begin([])
        s.synchronize()
        t0 = time.perf_counter()
        n = len(s.greedy_run(w, steps))
        s.synchronize()
        rates.append(n / (time.perf_counter() - t0))
    out[f"{wl} tok/s"] = float(np.median(rates[1:]))
    s.close(); w.close()
# int8 group-quantized weights: the step per kind at the 7B widths, one layer (quantized on the device from f32 weights)
c7 = shapes["llama2-7b"][0]
cfg = ck.Config(c7.dim, c7.hidden_dim, 1, c7.n_heads, c7.n_kv_heads, c7.vocab_size, c7.seq_len)
w32 = B.Weights(cfg, None, False, seed=2024)
w, s = B.Weights.quantized(w32, 64), B.RunState(cfg)
w32.close()
for pos in (0, 255):
    for kind in ("qkv", "attn", "wo", "ffn13", "ffn2", "cls", "argmax"):
        s.time_kind(kind, pos, w, reps=4)  # warm-up
        us = [s.time_kind(kind, pos, w, reps=16)[0] * 1e3 for _ in range(5)]
        out[f"q8 7B-width 1 layer pos {pos} {kind} us"] = float(np.median(us))
s.close(); w.close()
print(json.dumps(out), flush=True)
