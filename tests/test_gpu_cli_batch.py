"""The CLI's batch mode (`llama2 ckpt -b N`) end to end on the GPU, on the toy and the stories15M-2-layer shapes.

-b N runs the prompt once, forks it into N runstates, then steps them together (l2z_transformer_batch) and draws every
token on the device (l2z_sample_batch), sample i with numbers from its own generator seeded seed + i.  Checked here:
the token ids against an exact replay through the library, the same ids against the CPU oracle's logits, greedy
samples, the refusal of -b with -g, and that -b 1 is the run without -b byte for byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "llama2.zig_amd", "host")
EXE = os.path.join(HOST, "llama2")
TOK = os.path.join(ROOT, "tests", "golden", "tokenizer.bin")
TEXT = "a b c d e f g h"
# tests/test_gpu_batch_decode.py: a batched step's logits agree with the oracle's to |dz| <= ATOL + RTOL * |z|
LOGIT_RTOL = 5e-5
LOGIT_ATOL = 5e-5


@pytest.fixture(scope="module")
def H(B):
    L = C.CDLL(os.path.join(HOST, "libllama2_host.so"))
    fp = C.POINTER(C.c_float)
    L.l2zh_prng_open.restype = C.c_void_p
    L.l2zh_prng_open.argtypes = [C.c_uint64]
    L.l2zh_prng_close.argtypes = [C.c_void_p]
    L.l2zh_sample_top_p_rng.restype = C.c_size_t
    L.l2zh_sample_top_p_rng.argtypes = [fp, C.c_size_t, C.c_float, C.c_void_p, fp]
    L.l2zh_softmax.argtypes = [fp, C.c_size_t]
    L.l2zh_tokenizer_open.restype = C.c_void_p
    L.l2zh_tokenizer_open.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.l2zh_tokenizer_close.argtypes = [C.c_void_p]
    L.l2zh_tokenizer_encode.restype = C.c_long
    L.l2zh_tokenizer_encode.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), C.c_size_t]
    return L


def shape_cfg(ck, shape):
    if shape == "toy":
        return ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=96), False, 5
    return ck.Config(dim=288, hidden_dim=768, n_layers=2, n_heads=6, n_kv_heads=6, vocab_size=32000, seq_len=256), True, 15


@pytest.fixture(scope="module", params=["toy", "stories15M-2layers"])
def model(request, ck, tmp_path_factory):
    cfg, shared, seed_w = shape_cfg(ck, request.param)
    blob = ck.synth_blob(cfg, shared, seed_w)
    path = str(tmp_path_factory.mktemp(request.param) / "m.bin")
    ck.write_checkpoint(path, cfg, blob, shared)
    return request.param, cfg, shared, blob, path


def encode(H, cfg, text):
    err = C.create_string_buffer(128)
    t = H.l2zh_tokenizer_open(TOK.encode(), cfg.vocab_size, err, 128)
    assert t, err.value
    out = (C.c_int32 * 64)()
    n = H.l2zh_tokenizer_encode(t, text.encode(), len(text.encode()), out, 64)
    H.l2zh_tokenizer_close(t)
    assert n >= 4
    return [int(v) for v in out[:n]]


def run_cli(path, *args, env=None):
    r = subprocess.run([EXE, path, "-z", TOK, *args], capture_output=True, timeout=300,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return r


def sample_ids(r, nb):
    lines = {l.split(":")[0]: l for l in r.stderr.decode(errors="replace").splitlines() if l.startswith("tokens[")}
    return [[int(v) for v in lines[f"tokens[{i}]"].split(":", 1)[1].split()] for i in range(nb)]


def replay(gpu, H, cfg, path_blob, prompt, nb, n, temp, top_p, seed):
    """prefill + fork + transformer_batch + l2z_probs_read + the host's sample_top_p with Prng(seed + i): the ids each
    sample must print"""
    ck_cfg, shared, blob = path_blob
    w = gpu.Weights(cfg, blob, shared)
    states = [gpu.RunState(cfg) for _ in range(nb)]
    states[0].prefill([1] + prompt[:-1], 0, w)
    for s in states[1:]:
        gpu.runstate_fork(s, states[0], len(prompt))
    rngs = [H.l2zh_prng_open(seed + i) for i in range(nb)]
    ids = [list(prompt) for _ in range(nb)]
    alive = list(range(nb))
    for pos in range(len(prompt), n):
        if not alive:
            break
        gpu.transformer_batch([states[i] for i in alive], [ids[i][-1] for i in alive], [pos] * len(alive), w)
        for i in list(alive):
            pp = states[i].probs(temp)
            nxt = int(H.l2zh_sample_top_p_rng(pp.ctypes.data_as(C.POINTER(C.c_float)), cfg.vocab_size,
                                              C.c_float(top_p), rngs[i], None))
            ids[i].append(nxt)
            if nxt == 1:
                alive.remove(i)
    for r in rngs:
        H.l2zh_prng_close(r)
    for s in states:
        s.close()
    w.close()
    return ids


def test_batch_samples_equal_the_library_replay_and_the_oracle(gpu, ck, orc, H, model):
    """Exact: every sample's ids equal the replay through the library (the device sampler draws what the host sampler
    draws from l2z_probs_read's probabilities with the same number).

    Against the oracle (its stepped logits -> host softmax -> host sample_top_p, same numbers), a sample may diverge,
    but only at a draw whose number lies within B of a boundary of the truncated cdf.  B: the batched pass's logits are
    within d = ATOL + RTOL * max|z| of the oracle's (test_gpu_batch_decode.py).  A shift of every logit by at most d moves
    each probability by a factor within exp(+-2d/T), so every cdf boundary (a sum of probabilities <= 1) moves by at
    most 2d/T + O(d^2), and the scaled number r = coin * cumulative by at most 2d/T as well: 4d/T together.  The f32
    sums on the two sides round differently on different inputs: at most one half-ulp of a sum <= 1 (2^-25) per added
    candidate on each side, m * 2^-24 for m candidates.  B = 4d/T + m * 2^-24 (a bound, far above what occurs)."""
    shape, cfg, shared, blob, path = model
    prompt = encode(H, cfg, TEXT)
    nb, n, temp, top_p, seed = 4, 48, 1.0, 0.9, 2024
    r = run_cli(path, "-b", str(nb), "-t", str(temp), "-p", str(top_p), "-s", str(seed), "-n", str(n), "-i", TEXT,
                "--tokens")
    got = sample_ids(r, nb)
    want = replay(gpu, H, cfg, (cfg, shared, blob), prompt, nb, n, temp, top_p, seed)
    assert got == want
    out = r.stdout.decode(errors="replace")
    assert all(f"--- sample {i} ---" in out for i in range(nb))
    # against the oracle
    for i in range(nb):
        m = orc.Model(cfg.as_i32(), blob, shared)
        rng = H.l2zh_prng_open(seed + i)
        tok = 1
        for pos in range(len(got[i])):
            lg = m.transformer(tok, pos)
            nxt = got[i][pos]
            if pos >= len(prompt):
                pp = np.ascontiguousarray(lg / np.float32(temp), np.float32)
                H.l2zh_softmax(pp.ctypes.data_as(C.POINTER(C.c_float)), pp.size)
                mg = C.c_float(0)
                ref = int(H.l2zh_sample_top_p_rng(pp.ctypes.data_as(C.POINTER(C.c_float)), cfg.vocab_size,
                                                  C.c_float(top_p), rng, C.byref(mg)))
                if ref != nxt:
                    d = LOGIT_ATOL + LOGIT_RTOL * float(np.abs(lg).max())
                    n_cand = int(np.count_nonzero(pp >= (1 - top_p) / (cfg.vocab_size - 1)))
                    bound = 4 * d / temp + n_cand * 2.0 ** -24
                    print(f"{shape} sample {i}: diverges from the oracle at pos {pos} ({nxt} vs {ref}), "
                          f"cdf margin {mg.value:.3e} < bound {bound:.3e}")
                    assert mg.value < bound, (shape, i, pos, nxt, ref, mg.value, bound)
                    break
            tok = nxt
        H.l2zh_prng_close(rng)
        m.close()


def test_batch_greedy_samples_are_identical(gpu, model):
    _, cfg, _, _, path = model
    r = run_cli(path, "-b", "3", "-t", "0", "-n", "40", "-i", TEXT, "--tokens")
    ids = sample_ids(r, 3)
    assert ids[0] == ids[1] == ids[2] and len(ids[0]) > 8
    texts = r.stdout.decode(errors="replace").split("--- sample ")[1:]
    assert len(texts) == 3 and len({t.split("\n", 1)[1] for t in texts}) == 1


def test_batch_with_gpus_is_refused(gpu, model):
    _, _, _, _, path = model
    r = subprocess.run([EXE, path, "-z", TOK, "-b", "2", "-g", "2"], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"shard groups are not batched" in r.stderr


def test_batch_of_one_is_the_run_without_batch(gpu, model):
    _, _, _, _, path = model
    for extra in ((), ("-i", TEXT)):
        a = run_cli(path, "-t", "1.0", "-p", "0.9", "-s", "31", "-n", "40", *extra)
        b = run_cli(path, "-t", "1.0", "-p", "0.9", "-s", "31", "-n", "40", "-b", "1", *extra)
        assert a.stdout == b.stdout and len(a.stdout) > 0
