"""llama2.c "legacy v0" checkpoint format, as the reference reads it.

Layout (cited against /root/reference/src/main.zig):
  * 28-byte header = ConfigReader, 7 x i32 little endian (main.zig:17-25, read
    at :941).  vocab_size < 0 signals an UNSHARED classifier (main.zig:943-944).
  * one flat f32 blob carved by Weights.init in a fixed order (main.zig:85-112),
    including the freq_cis_real/imag region that is skipped but never read.

No real checkpoint exists in the build image, so this module also produces
seeded synthetic blobs.  The generator is specified in DESIGN.md ("Synthetic
checkpoints") and implemented three times -- here (numpy), in the CPU oracle
(oracle/llama2_oracle.c: orc_synth_*) and on the device (csrc/misc_kernels.hip: synth_fill_kernel) --
tests check the three agree bit for bit.
"""
from __future__ import annotations

import dataclasses
import struct
from typing import Iterator, NamedTuple

import numpy as np

HEADER_BYTES = 28


@dataclasses.dataclass(frozen=True)
class Config:
    """main.zig:41-49 (vocab_size already abs()'d)."""

    dim: int
    hidden_dim: int
    n_layers: int
    n_heads: int
    n_kv_heads: int
    vocab_size: int
    seq_len: int

    @property
    def head_size(self) -> int:
        return self.dim // self.n_heads

    @property
    def kv_dim(self) -> int:
        return (self.dim * self.n_kv_heads) // self.n_heads

    @property
    def kv_mul(self) -> int:
        return self.n_heads // self.n_kv_heads

    def as_i32(self) -> np.ndarray:
        return np.array(dataclasses.astuple(self), dtype=np.int32)


# The shapes BASELINE.json names.
STORIES15M = Config(288, 768, 6, 6, 6, 32000, 256)
STORIES110M = Config(768, 2048, 12, 12, 12, 32000, 1024)
# llama2.c's public stories42M checkpoint: not a BASELINE config, but a model the reference runs whose hidden_dim
# (1376 = 4 * 344, 344 = 5 * 64 + 24) is not a whole number of 64-lane float4 steps: the mat-vec's partial last step
STORIES42M = Config(512, 1376, 8, 8, 8, 32000, 1024)
LLAMA2_7B = Config(4096, 11008, 32, 32, 32, 32000, 2048)


class Tensor(NamedTuple):
    name: str
    offset: int  # in f32, from the start of the blob
    shape: tuple  # logical shape
    scale: np.float32  # synthetic generator: value = bias + scale * r
    bias: np.float32

    @property
    def count(self) -> int:
        n = 1
        for s in self.shape:
            n *= s
        return n


def tensor_table(c: Config, shared_weights: bool) -> list[Tensor]:
    """The Weights.init pointer walk (main.zig:85-112) as a table."""
    L, dim, hid, V, S = c.n_layers, c.dim, c.hidden_dim, c.vocab_size, c.seq_len
    hs, kvd = c.head_size, c.kv_dim
    f = np.float32
    s_dim = np.sqrt(f(3.0) / f(dim), dtype=np.float32)
    s_hid = np.sqrt(f(3.0) / f(hid), dtype=np.float32)
    s_emb = f(2.0) * s_dim
    rows = [
        ("token_embedding_table", (V, dim), s_emb, f(0)),
        ("rms_att_weight", (L, dim), f(0.1), f(1)),
        ("wq", (L, dim, dim), s_dim, f(0)),
        ("wk", (L, kvd, dim), s_dim, f(0)),
        ("wv", (L, kvd, dim), s_dim, f(0)),
        ("wo", (L, dim, dim), s_dim, f(0)),
        ("rms_ffn_weight", (L, dim), f(0.1), f(1)),
        ("w1", (L, hid, dim), s_dim, f(0)),
        ("w2", (L, dim, hid), s_hid, f(0)),
        ("w3", (L, hid, dim), s_dim, f(0)),
        ("rms_final_weight", (dim,), f(0.1), f(1)),
        ("freq_cis_real", (S * hs // 2,), f(1), f(0)),
        ("freq_cis_imag", (S * hs // 2,), f(1), f(0)),
    ]
    if not shared_weights:
        rows.append(("wcls", (V, dim), s_emb, f(0)))
    out, off = [], 0
    for name, shape, scale, bias in rows:
        t = Tensor(name, off, shape, f(scale), f(bias))
        out.append(t)
        off += t.count
    return out


def weights_count(c: Config, shared_weights: bool) -> int:
    t = tensor_table(c, shared_weights)[-1]
    return t.offset + t.count


def file_size(c: Config, shared_weights: bool) -> int:
    return HEADER_BYTES + 4 * weights_count(c, shared_weights)


def carve(c: Config, blob: np.ndarray, shared_weights: bool) -> dict[str, np.ndarray]:
    """Views into the blob, one per tensor (Weights.init)."""
    assert blob.dtype == np.float32 and blob.ndim == 1
    out = {}
    for t in tensor_table(c, shared_weights):
        out[t.name] = blob[t.offset : t.offset + t.count].reshape(t.shape)
    if shared_weights:
        out["wcls"] = out["token_embedding_table"]  # main.zig:112
    return out


def _mix64(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def synth_values(base_idx: int, count: int, seed: int, scale, bias) -> np.ndarray:
    """value(idx) = bias + scale * r(idx, seed); r on a 2^-22 grid in [-1, 1)."""
    with np.errstate(over="ignore"):
        idx = np.arange(base_idx, base_idx + count, dtype=np.uint64)
        z = _mix64(idx + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15))
    u = (z >> np.uint64(41)).astype(np.float32)  # 23 bits, exact
    r = u * np.float32(2.0**-22) - np.float32(1.0)  # exact
    return (np.float32(bias) + np.float32(scale) * r).astype(np.float32)


def synth_blob(c: Config, shared_weights: bool, seed: int) -> np.ndarray:
    blob = np.empty(weights_count(c, shared_weights), dtype=np.float32)
    for t in tensor_table(c, shared_weights):
        chunk = 1 << 22
        for lo in range(0, t.count, chunk):
            n = min(chunk, t.count - lo)
            blob[t.offset + lo : t.offset + lo + n] = synth_values(
                t.offset + lo, n, seed, t.scale, t.bias
            )
    return blob


def write_checkpoint(path, c: Config, blob: np.ndarray, shared_weights: bool) -> None:
    assert blob.dtype == np.float32 and blob.size == weights_count(c, shared_weights)
    hdr = list(dataclasses.astuple(c))
    if not shared_weights:
        hdr[5] = -hdr[5]  # main.zig:943: negative vocab = unshared classifier
    with open(path, "wb") as f:
        f.write(struct.pack("<7i", *hdr))
        f.write(blob.astype("<f4", copy=False).tobytes())


def read_checkpoint(path, mmap: bool = True):
    """Returns (Config, shared_weights, blob[f32]).  main.zig:936-967."""
    with open(path, "rb") as f:
        hdr = struct.unpack("<7i", f.read(HEADER_BYTES))
    shared = hdr[5] > 0
    c = Config(hdr[0], hdr[1], hdr[2], hdr[3], hdr[4], abs(hdr[5]), hdr[6])
    if mmap:
        blob = np.memmap(path, dtype="<f4", mode="r", offset=HEADER_BYTES)
    else:
        blob = np.fromfile(path, dtype="<f4", offset=HEADER_BYTES)
    need = weights_count(c, shared)
    if blob.size < need:
        raise ValueError(f"checkpoint too small: {blob.size} f32 < {need}")
    return c, shared, blob[:need]


def iter_configs() -> Iterator[tuple[str, Config, bool]]:
    yield "stories15M", STORIES15M, True
    yield "stories110M", STORIES110M, True
    yield "stories42M", STORIES42M, True
    yield "llama2-7b", LLAMA2_7B, False


# ---------------------------------------------------------------------------
# llama2.c "version 2" checkpoints: int8 group-quantized weights
#
# 256-byte header, little endian: u32 magic 0x616b3432, i32 version 2, the seven config ints, u8 shared_classifier at
# byte 36, i32 group_size at byte 37 (unaligned), zero padding.  Body: f32 rms_att_weight [L, dim], rms_ffn_weight
# [L, dim], rms_final_weight [dim], then every quantized tensor as its int8 values followed by its f32 scales (one per
# group): the token embedding, wq, wk, wv, wo, w1, w2, w3 (each layer by layer), wcls unless shared.
V2_MAGIC = 0x616B3432
V2_HEADER_BYTES = 256
V2_QUANTIZED = ("token_embedding_table", "wq", "wk", "wv", "wo", "w1", "w2", "w3", "wcls")
V2_GROUP_SIZES = (32, 64)


def quantize_q80(w, gs: int):
    """Group quantization by the WEIGHT rule: per group of gs consecutive elements s = max|v| / 127 (one f32 division),
    q = round-half-to-even(v / s) (one f32 division, then np.rint) as int8; a group whose scale is 0 has all q = 0.
    Returns (q int8 of w's shape, s f32 [w.size // gs]).  Non-finite inputs are unspecified."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    assert w.size % gs == 0
    g = w.reshape(-1, gs)
    s = (np.abs(g).max(axis=1) / np.float32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        quot = (g / s[:, None]).astype(np.float32)
    q = np.where(s[:, None] > 0, np.rint(quot), np.float32(0)).astype(np.int8)
    return q.reshape(w.shape), s


class V2Tensor(NamedTuple):
    name: str
    shape: tuple     # (layers, rows, cols)
    q_offset: int    # bytes from the start of the body
    s_offset: int

    @property
    def count(self) -> int:
        return self.shape[0] * self.shape[1] * self.shape[2]


class V2Layout(NamedTuple):
    gs: int
    norms: dict      # name -> (byte offset, shape) of the three f32 tensors
    tensors: dict    # name -> V2Tensor
    total: int       # bytes of the body


def v2_layout(c: Config, shared: bool, gs: int) -> V2Layout:
    """Byte offsets of everything in a version-2 body (csrc/q8_layout.h computes the same)."""
    if gs not in V2_GROUP_SIZES:
        raise ValueError(f"group size {gs}: 32 or 64")
    if c.dim % gs or c.hidden_dim % gs:
        raise ValueError(f"dim {c.dim} and hidden_dim {c.hidden_dim} must be multiples of the group size {gs}")
    L, dim, hid, V, kvd = c.n_layers, c.dim, c.hidden_dim, c.vocab_size, c.kv_dim
    off = 0
    norms = {}
    for name, shape in (("rms_att_weight", (L, dim)), ("rms_ffn_weight", (L, dim)), ("rms_final_weight", (dim,))):
        norms[name] = (off, shape)
        off += 4 * int(np.prod(shape))
    shapes = {"token_embedding_table": (1, V, dim), "wq": (L, dim, dim), "wk": (L, kvd, dim), "wv": (L, kvd, dim),
              "wo": (L, dim, dim), "w1": (L, hid, dim), "w2": (L, dim, hid), "w3": (L, hid, dim), "wcls": (1, V, dim)}
    tensors = {}
    for name in V2_QUANTIZED:
        if name == "wcls" and shared:
            continue
        n = shapes[name][0] * shapes[name][1] * shapes[name][2]
        tensors[name] = V2Tensor(name, shapes[name], off, off + n)
        off += n + 4 * (n // gs)
    return V2Layout(gs, norms, tensors, off)


def v2_header(c: Config, shared: bool, gs: int) -> bytes:
    hdr = struct.pack("<Ii7i", V2_MAGIC, 2, *dataclasses.astuple(c)) + struct.pack("<B", 1 if shared else 0) + struct.pack("<i", gs)
    return hdr + bytes(V2_HEADER_BYTES - len(hdr))


def v2_body_from_f32(c: Config, blob: np.ndarray, shared: bool, gs: int) -> np.ndarray:
    """The version-2 body (uint8) of an f32 blob in the version-0 order: the norms copied, the matrices quantized."""
    lay = v2_layout(c, shared, gs)
    t = carve(c, np.ascontiguousarray(blob, dtype=np.float32), shared)
    body = np.zeros(lay.total, np.uint8)
    for name, (off, shape) in lay.norms.items():
        body[off : off + 4 * int(np.prod(shape))] = np.ascontiguousarray(t[name], dtype="<f4").reshape(-1).view(np.uint8)
    for name, vt in lay.tensors.items():
        q, s = quantize_q80(t[name], gs)
        body[vt.q_offset : vt.q_offset + vt.count] = q.reshape(-1).view(np.uint8)
        body[vt.s_offset : vt.s_offset + 4 * s.size] = s.astype("<f4").view(np.uint8)
    return body


def v2_carve(c: Config, body: np.ndarray, shared: bool, gs: int) -> dict:
    """Views into a version-2 body: the three norms as f32 arrays, every quantized tensor as (q int8 [L, rows, cols],
    s f32 [L, rows, cols // gs]); "wcls" is the embedding table's pair where the file shares them."""
    lay = v2_layout(c, shared, gs)
    body = np.asarray(body).view(np.uint8).reshape(-1)
    if body.size < lay.total:
        raise ValueError(f"version-2 body too small: {body.size} bytes < {lay.total}")
    out = {}
    for name, (off, shape) in lay.norms.items():
        out[name] = body[off : off + 4 * int(np.prod(shape))].view("<f4").reshape(shape)
    for name, vt in lay.tensors.items():
        L, rows, cols = vt.shape
        out[name] = (body[vt.q_offset : vt.q_offset + vt.count].view(np.int8).reshape(vt.shape),
                     body[vt.s_offset : vt.s_offset + 4 * (vt.count // gs)].view("<f4").reshape(L, rows, cols // gs))
    if shared:
        out["wcls"] = out["token_embedding_table"]
    return out


def write_checkpoint_v2(path, c: Config, body: np.ndarray, shared: bool, gs: int) -> None:
    lay = v2_layout(c, shared, gs)
    body = np.asarray(body).view(np.uint8).reshape(-1)
    assert body.size == lay.total
    with open(path, "wb") as f:
        f.write(v2_header(c, shared, gs))
        f.write(body.tobytes())


def read_checkpoint_v2(path, mmap: bool = True):
    """Returns (Config, shared_classifier, group_size, body[uint8])."""
    with open(path, "rb") as f:
        hdr = f.read(V2_HEADER_BYTES)
    if len(hdr) < V2_HEADER_BYTES:
        raise ValueError("version-2 checkpoint: header too short")
    magic, version = struct.unpack_from("<Ii", hdr, 0)
    if magic != V2_MAGIC or version != 2:
        raise ValueError(f"not a version-2 checkpoint (magic {magic:#x}, version {version})")
    c = Config(*struct.unpack_from("<7i", hdr, 8))
    shared = hdr[36] != 0
    (gs,) = struct.unpack_from("<i", hdr, 37)
    lay = v2_layout(c, shared, gs)
    if mmap:
        body = np.memmap(path, dtype=np.uint8, mode="r", offset=V2_HEADER_BYTES)
    else:
        body = np.fromfile(path, dtype=np.uint8, offset=V2_HEADER_BYTES)
    if body.size < lay.total:
        raise ValueError(f"version-2 checkpoint too small: body has {body.size} bytes, config needs {lay.total}")
    return c, shared, gs, body[: lay.total]
