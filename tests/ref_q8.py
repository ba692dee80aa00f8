"""CPU reference of the int8 group-quantized pass, numpy, in two arithmetic modes:

  "f32"  every operation rounds to f32 and every sum runs sequentially, in runq.c's order (val += (f32(ival) * ws) * xs
         group by group; the rmsnorm, the attention scores, the softmax and the weighted sums element by element);
  "f64"  the same pass with everything that is not DEFINED in f32 carried in float64.

What is defined in f32 is the same in both: the quantization rule itself (scale = max / 127 and the quotient are single f32
divisions of the f32 input; a float64 activation is rounded to f32 first), the embedding row f32(q) * s, and the RoPE table
(the runstate's: f32 powf / cosf / sinf).  The integer sums are exact in both.  The pass is discontinuous -- an activation
within f32 noise of a rounding boundary may land on either side --, so the modes agree to f32 noise at almost every position
and to a few 1e-3 where one element flipped (tests/test_ref_q8_cpu.py measures it).
"""
import numpy as np

f32 = np.float32


def quantize_act(x, gs, margins=None):
    """The ACTIVATION rule: s = max|v| / 127 (one f32 division), q = round-half-away-from-zero of the f32 quotient v / s.
    The rounding is done in float64 FROM the f32 quotient (exact there), never as floor(|v| + 0.5) in f32, which differs at
    0.49999997.  margins: a list that gets the smallest distance of a quotient of this call to a rounding boundary
    (how safe the call is from landing on the other side under another summation order)."""
    x = np.ascontiguousarray(x, dtype=f32).reshape(-1, gs)
    s = (np.abs(x).max(axis=1) / f32(127.0)).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        quot = (x / s[:, None]).astype(f32).astype(np.float64)
    r = np.sign(quot) * np.floor(np.abs(quot) + 0.5)
    if margins is not None:
        margins.append(float(np.min(np.abs(np.abs(quot[np.isfinite(quot)]) % 1.0 - 0.5), initial=0.5)))
    q = np.where(s[:, None] > 0, r, 0.0).astype(np.int8)
    return q.reshape(-1), s


def group_sums(wq, xq, gs):
    """I[i, g]: the exact integer sums of a [d, n] int8 matrix against an int8 vector, per group."""
    d, n = wq.shape
    prod = wq.astype(np.int32).reshape(d, n // gs, gs) * xq.astype(np.int32).reshape(1, n // gs, gs)
    return prod.sum(axis=2, dtype=np.int64)


def matvec_terms64(wq, ws, xq, xs, gs):
    """The terms f32(I) * ws * xs of every output in float64 (no rounding): [d, n // gs]."""
    I = group_sums(wq, xq, gs).astype(np.float64)
    return I * ws.astype(np.float64).reshape(I.shape) * xs.astype(np.float64)[None, :]


def matvec(wq, ws, xq, xs, gs, mode):
    I = group_sums(wq, xq, gs)
    ws = ws.reshape(I.shape)
    if mode == "f64":
        return matvec_terms64(wq, ws, xq, xs, gs).sum(axis=1)
    val = np.zeros(I.shape[0], f32)
    for g in range(I.shape[1]):  # runq.c: val += ((float) ival) * w->s[..] * x->s[..]
        val = (val + (I[:, g].astype(f32) * ws[:, g]) * xs[g]).astype(f32)
    return val


def rope_table(cfg):
    """(seq_len, head_size / 2) cos and sin, evaluated in f32 as the runstate does."""
    hs = cfg.head_size
    j = np.arange(hs // 2, dtype=f32)
    freq = (f32(1.0) / np.power(f32(10000.0), (f32(2.0) * j) / f32(hs), dtype=f32)).astype(f32)
    val = (np.arange(cfg.seq_len, dtype=f32)[:, None] * freq[None, :]).astype(f32)
    return np.cos(val, dtype=f32), np.sin(val, dtype=f32)


class Q8Model:
    """One sequence of the quantized pass.  t: checkpoint.v2_carve(...)'s dictionary."""

    def __init__(self, cfg, t, gs, mode):
        assert mode in ("f32", "f64")
        self.c, self.t, self.gs, self.mode = cfg, t, gs, mode
        self.ft = f32 if mode == "f32" else np.float64
        self.kc = np.zeros((cfg.n_layers, cfg.seq_len, cfg.kv_dim), self.ft)
        self.vc = np.zeros((cfg.n_layers, cfg.seq_len, cfg.kv_dim), self.ft)
        self.cos, self.sin = rope_table(cfg)
        self.margins = []   # of every activation quantization so far: quantize_act's

    def _seq_sum(self, a, axis=0):
        if self.mode == "f64":
            return a.sum(axis=axis)
        return np.take(np.cumsum(a, axis=axis, dtype=f32), -1, axis=axis)  # (cumsum adds one by one, in order)

    def rmsnorm(self, x, w):
        ft = self.ft
        ss = self._seq_sum((x * x).astype(ft)) / ft(x.size)
        ss = ft(ss + ft(1e-5))
        ss = ft(ft(1.0) / np.sqrt(ss, dtype=ft))
        return ((x * ss).astype(ft) * w.astype(ft)).astype(ft)

    def qmatvec(self, name, l, x):
        q, s = self.t[name]
        xq, xs = quantize_act(np.asarray(x).astype(f32), self.gs, self.margins)
        return matvec(q[l], s[l], xq, xs, self.gs, self.mode).astype(self.ft)

    def transformer(self, token, pos):
        c, t, ft, gs = self.c, self.t, self.ft, self.gs
        hs, kvd, kv_mul = c.head_size, c.kv_dim, c.kv_mul
        eq, es = t["token_embedding_table"]
        x = (eq[0, token].astype(f32) * np.repeat(es[0, token], gs)).astype(f32).astype(ft)  # f32(q) * s, one rounding
        cs, sn = self.cos[pos].astype(ft), self.sin[pos].astype(ft)
        for l in range(c.n_layers):
            xb = self.rmsnorm(x, t["rms_att_weight"][l])
            xq, xs = quantize_act(xb.astype(f32), gs, self.margins)
            q = matvec(*[t["wq"][i][l] for i in (0, 1)], xq, xs, gs, self.mode).astype(ft)
            k = matvec(*[t["wk"][i][l] for i in (0, 1)], xq, xs, gs, self.mode).astype(ft)
            v = matvec(*[t["wv"][i][l] for i in (0, 1)], xq, xs, gs, self.mode).astype(ft)

            def rot(a):  # main.zig:336-351: pairs (i, i + 1), the angle of (i % head_size) / 2
                a = a.reshape(-1, hs // 2, 2)
                a0, a1 = a[:, :, 0], a[:, :, 1]
                r0 = ((a0 * cs).astype(ft) - (a1 * sn).astype(ft)).astype(ft)
                r1 = ((a0 * sn).astype(ft) + (a1 * cs).astype(ft)).astype(ft)
                return np.stack([r0, r1], axis=2).reshape(-1)

            q, k = rot(q), rot(k)
            self.kc[l, pos], self.vc[l, pos] = k, v
            out = np.zeros(c.dim, ft)
            for h in range(c.n_heads):
                kh = (h // kv_mul) * hs
                K = self.kc[l, : pos + 1, kh : kh + hs]
                V = self.vc[l, : pos + 1, kh : kh + hs]
                att = self._seq_sum((K * q[None, h * hs : (h + 1) * hs]).astype(ft), axis=1)
                att = (att / np.sqrt(ft(hs), dtype=ft)).astype(ft)
                e = np.exp((att - att.max()).astype(ft), dtype=ft)
                p = (e / self._seq_sum(e)).astype(ft)
                out[h * hs : (h + 1) * hs] = self._seq_sum((p[:, None] * V).astype(ft), axis=0)
            x = (x + self.qmatvec("wo", l, out)).astype(ft)
            xb = self.rmsnorm(x, t["rms_ffn_weight"][l])
            xq, xs = quantize_act(xb.astype(f32), gs, self.margins)
            h1 = matvec(*[t["w1"][i][l] for i in (0, 1)], xq, xs, gs, self.mode).astype(ft)
            h3 = matvec(*[t["w3"][i][l] for i in (0, 1)], xq, xs, gs, self.mode).astype(ft)
            sig = (ft(1.0) / (ft(1.0) + np.exp(-h1, dtype=ft)).astype(ft)).astype(ft)
            hb = ((h1 * sig).astype(ft) * h3).astype(ft)
            x = (x + self.qmatvec("w2", l, hb)).astype(ft)
        x = self.rmsnorm(x, t["rms_final_weight"])
        return self.qmatvec("wcls", 0, x)


def run_positions(ck, cfg, body, shared, gs, tokens, mode):
    """Logits [len(tokens), vocab] of tokens[p] at position p, and the model (its kc / vc hold every layer's K / V rows)."""
    m = Q8Model(cfg, ck.v2_carve(cfg, body, shared, gs), gs, mode)
    z = np.stack([m.transformer(int(tok), p) for p, tok in enumerate(tokens)])
    return z, m


def greedy(ck, cfg, body, shared, gs, prompt, n_steps, mode="f64"):
    """The ids of the greedy loop (main.zig:987-1042 at temperature 0) and the top-2 margin of every step's logits."""
    m = Q8Model(cfg, ck.v2_carve(cfg, body, shared, gs), gs, mode)
    tok, ids, margins, zs = 1, [], [], []
    for pos in range(n_steps):
        z = m.transformer(tok, pos)
        top = np.sort(z)[-2:]
        margins.append(float(top[1] - top[0]))
        nxt = int(prompt[pos]) if pos < len(prompt) else int(np.argmax(z))
        ids.append(nxt)
        zs.append(z)
        tok = nxt
    return np.array(ids, np.int32), np.array(margins), np.stack(zs)
