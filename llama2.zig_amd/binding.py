"""ctypes binding over libllama2_hip_test.so (include/llama2_hip.h + include/llama2_hip_test.h; the product library
libllama2_hip.so exports the first header only).

This is what tests/ and bench.py call: every compute path goes through the
C ABI into the hand-written HIP kernels.  There is no Python or CPU fallback
here -- if the library is missing or no gfx950 device is present the calls
raise (`L2ZError`), they never silently compute on the host.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product library (exports include/llama2_hip.h only: what a host links) and the library this binding loads: the same
# objects with the test / measurement entry points of include/llama2_hip_test.h exported as well (csrc/Makefile).
PRODUCT_LIB_PATH = os.path.join(_HERE, "libllama2_hip.so")
LIB_PATH = os.environ.get("L2Z_LIB") or os.path.join(_HERE, "libllama2_hip_test.so")  # L2Z_LIB: A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "llama2_hip.h")
TEST_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "llama2_hip_test.h")

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_OOM, ERR_COMM, ERR_STATE = 0, -1, -2, -3, -4, -5, -6
COMM_ID_BYTES = 128
COMM_IPC_BYTES = 64
KINDS = ["qkv", "attn", "wo", "ffn13", "ffn2", "cls", "argmax", "gather"]


class L2ZError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"llama2_hip error {code}: {msg}")
        self.code = code


class L2ZConfig(C.Structure):
    """src/main.zig:17-25 ConfigReader layout."""

    _fields_ = [(n, C.c_int32) for n in
                ("dim", "hidden_dim", "n_layers", "n_heads", "n_kv_heads", "vocab_size", "seq_len")]


def declared_symbols(which: str = "all") -> list[str]:
    """Every function the headers declare (for the export check): the drop-in boundary
    include/llama2_hip.h ("product"), the test / measurement entry points of
    include/llama2_hip_test.h ("test"), or both."""
    paths = {"product": [HEADER_PATH], "test": [TEST_HEADER_PATH],
             "all": [HEADER_PATH, TEST_HEADER_PATH]}[which]
    out = set()
    for path in paths:
        txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        out |= set(re.findall(r"\b(l2z_[a-z0-9_]+)\s*\(", txt))
    return sorted(out)


_lib = None


def lib():
    """Load the library (raises if it was not built -- run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    fp, sz, vp = C.POINTER(C.c_float), C.c_size_t, C.c_void_p
    cfgp = C.POINTER(L2ZConfig)
    i32p, ip = C.POINTER(C.c_int32), C.POINTER(C.c_int)
    L.l2z_last_error.restype = C.c_char_p
    L.l2z_device_count.argtypes = [ip]
    L.l2z_device_info.argtypes = [C.c_int, C.c_char_p, sz, ip, C.POINTER(C.c_uint64)]
    L.l2z_weights_init.argtypes = [cfgp, fp, sz, C.c_int, vp, C.POINTER(vp)]
    L.l2z_weights_init_synthetic.argtypes = [cfgp, C.c_int, C.c_uint64, vp, C.POINTER(vp)]
    L.l2z_weights_read.argtypes = [vp, sz, sz, fp]
    L.l2z_weights_free.argtypes = [vp]
    L.l2z_weights_free.restype = None
    L.l2z_runstate_init.argtypes = [cfgp, vp, C.POINTER(vp)]
    L.l2z_runstate_free.argtypes = [vp]
    L.l2z_runstate_free.restype = None
    L.l2z_transformer.argtypes = [C.c_int, C.c_int, cfgp, vp, vp]
    L.l2z_argmax.argtypes = [vp, ip]
    L.l2z_logits_read.argtypes = [vp, fp]
    L.l2z_probs_read.argtypes = [vp, C.c_float, fp]
    L.l2z_runstate_read.argtypes = [vp, C.c_char_p, sz, sz, fp]
    L.l2z_prefill.argtypes = [i32p, C.c_int, C.c_int, cfgp, vp, vp]
    if hasattr(L, "l2z_score"):  # (an older build loaded through L2Z_LIB lacks it)
        L.l2z_score.argtypes = [i32p, C.c_int, C.c_int, i32p, cfgp, vp, vp, fp, i32p]
        L.l2z_score_slab_set.argtypes = [vp, C.c_int]
    if hasattr(L, "l2z_verify"):
        L.l2z_verify.argtypes = [i32p, C.c_int, C.c_int, cfgp, vp, vp, i32p, ip]
        L.l2z_verify_logits_read.argtypes = [vp, C.c_int, fp]
        L.l2z_verify_time.argtypes = [i32p, C.c_int, C.c_int, cfgp, vp, vp, C.c_int, C.POINTER(C.c_double)]
    if hasattr(L, "l2z_verify_sample"):
        L.l2z_verify_sample.argtypes = [i32p, C.c_int, C.c_int, C.c_float, C.c_float, fp, cfgp, vp, vp, i32p, ip]
        L.l2z_verify_sample_time.argtypes = [i32p, C.c_int, C.c_int, C.c_float, C.c_float, fp, cfgp, vp, vp, C.c_int,
                                             C.POINTER(C.c_double)]
    L.l2z_transformer_batch.argtypes = [C.c_int, i32p, i32p, cfgp, C.POINTER(vp), vp]
    L.l2z_argmax_batch.argtypes = [C.c_int, C.POINTER(vp), i32p]
    L.l2z_batch_time.argtypes = [C.c_int, i32p, i32p, cfgp, C.POINTER(vp), vp, C.c_int, C.POINTER(C.c_double)]
    L.l2z_sample_batch.argtypes = [C.c_int, C.POINTER(vp), fp, fp, fp, i32p]
    L.l2z_runstate_fork.argtypes = [vp, vp, C.c_int]
    if hasattr(L, "l2z_prefill_batch"):
        L.l2z_prefill_batch.argtypes = [C.c_int, i32p, i32p, i32p, cfgp, C.POINTER(vp), vp]
    if hasattr(L, "l2z_transformer_wide"):
        L.l2z_transformer_wide.argtypes = [C.c_int, i32p, i32p, cfgp, C.POINTER(vp), vp, i32p]
    if hasattr(L, "l2z_wide_run"):
        L.l2z_wide_run.argtypes = [C.c_int, i32p, i32p, C.c_int, fp, fp, fp, cfgp, C.POINTER(vp), vp, i32p]
    if hasattr(L, "l2z_verify_batch"):
        L.l2z_verify_batch.argtypes = [C.c_int, i32p, i32p, i32p, fp, fp, fp, cfgp, C.POINTER(vp), vp, i32p, i32p]
    if hasattr(L, "l2z_verify_wide"):
        L.l2z_verify_wide.argtypes = [C.c_int, i32p, i32p, i32p, fp, fp, fp, cfgp, C.POINTER(vp), vp, i32p, i32p]
    if hasattr(L, "l2z_step_mixed"):
        L.l2z_step_mixed.argtypes = [C.c_int, i32p, i32p, i32p, fp, fp, fp, cfgp, C.POINTER(vp), vp, i32p]
    if hasattr(L, "l2z_kvpool_init"):
        L.l2z_kvpool_init.argtypes = [cfgp, C.c_int, C.POINTER(vp)]
        L.l2z_kvpool_free.argtypes = [vp]
        L.l2z_kvpool_info.argtypes = [vp, ip, ip, C.POINTER(C.c_uint64)]
        L.l2z_runstate_init_paged.argtypes = [cfgp, vp, C.POINTER(vp)]
        L.l2z_runstate_pages.argtypes = [vp, ip, i32p, C.c_int]
        L.l2z_runstate_trim.argtypes = [vp, C.c_int]
    if hasattr(L, "l2z_verify_tree"):
        L.l2z_verify_tree.argtypes = [i32p, i32p, C.c_int, C.c_int, C.c_float, C.c_float, fp, cfgp, vp, vp, i32p, i32p, ip]
        L.l2z_verify_tree_time.argtypes = [i32p, i32p, C.c_int, C.c_int, C.c_float, C.c_float, fp, cfgp, vp, vp, C.c_int,
                                           C.POINTER(C.c_double)]
    if hasattr(L, "l2z_sample_run"):
        L.l2z_sample_run.argtypes = [cfgp, vp, vp, C.c_int, C.c_float, C.c_float, fp, i32p, ip]
    if hasattr(L, "l2z_weights_init_q8"):  # int8 group-quantized weights (PREVIEW; include/llama2_hip_test.h)
        i8p = C.POINTER(C.c_int8)
        L.l2z_weights_init_q8.argtypes = [cfgp, vp, sz, C.c_int, C.c_int, vp, C.POINTER(vp)]
        L.l2z_weights_init_q8_from.argtypes = [vp, C.c_int, C.POINTER(vp)]
        L.l2z_weights_q8_read.argtypes = [vp, C.c_char_p, C.c_int, i8p, fp]
        L.l2z_q8_quantize.argtypes = [fp, sz, C.c_int, i8p, fp]
        L.l2z_q8_matmul.argtypes = [fp, i8p, fp, i8p, fp, sz, sz, C.c_int]
    if hasattr(L, "l2z_q8_matvec_case"):
        L.l2z_q8_matvec_case.argtypes = [C.POINTER(Q8Case)]
    if hasattr(L, "l2z_prefill_q8"):  # their batched prompt pass (PREVIEW)
        i8p = C.POINTER(C.c_int8)
        L.l2z_prefill_q8.argtypes = [i32p, C.c_int, C.c_int, cfgp, vp, vp]
        L.l2z_q8_quantize_rows.argtypes = [fp, C.c_int, sz, fp, C.c_int, i8p, fp]
        L.l2z_q8_gemm.argtypes = [fp, i8p, fp, C.c_int, i8p, fp, sz, sz, C.c_int]
    if hasattr(L, "l2z_transformer_batch_q8"):  # their batched step and verify pass (PREVIEW)
        L.l2z_transformer_batch_q8.argtypes = [C.c_int, i32p, i32p, cfgp, C.POINTER(vp), vp]
        L.l2z_verify_q8.argtypes = [i32p, C.c_int, C.c_int, C.c_float, C.c_float, fp, cfgp, vp, vp, i32p, ip]
        L.l2z_batch_q8_time.argtypes = [C.c_int, i32p, i32p, cfgp, C.POINTER(vp), vp, C.c_int, C.POINTER(C.c_double)]
        L.l2z_verify_q8_time.argtypes = [i32p, C.c_int, C.c_int, C.c_float, C.c_float, fp, cfgp, vp, vp, C.c_int,
                                         C.POINTER(C.c_double)]
    L.l2z_logits_write.argtypes = [vp, fp]
    L.l2z_sample_time.argtypes = [C.c_int, C.POINTER(vp), fp, fp, fp, C.c_int, C.POINTER(C.c_double)]
    L.l2z_greedy_begin.argtypes = [vp, i32p, C.c_int]
    L.l2z_greedy_run.argtypes = [cfgp, vp, vp, C.c_int, i32p, ip]
    L.l2z_profile_forward.argtypes = [C.c_int, C.c_int, cfgp, vp, vp, C.POINTER(C.c_double), ip,
                                      C.c_int]
    L.l2z_stream_read_probe.argtypes = [vp, vp, sz, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(L, "l2z_d2d_copy_probe"):
        L.l2z_d2d_copy_probe.argtypes = [vp, vp, sz, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.l2z_kind_name.argtypes = [C.c_int, C.c_char_p, sz]
    L.l2z_time_kind.argtypes = [C.c_int, C.c_int, cfgp, vp, vp, C.c_int, C.POINTER(C.c_double), ip]
    L.l2z_synchronize.argtypes = [vp]
    L.l2z_matmul.argtypes = [fp, fp, fp, sz, sz]
    L.l2z_matmul_fused.argtypes = [C.c_int, C.POINTER(fp), fp, C.POINTER(fp), sz, sz]
    L.l2z_rmsnorm.argtypes = [fp, fp, fp, sz]
    L.l2z_softmax.argtypes = [fp, sz]
    L.l2z_vector_dot_product.argtypes = [fp, fp, fp, sz]
    L.l2z_vector_weighted_sum_rows.argtypes = [fp, sz, fp, sz, sz, fp, sz]
    L.l2z_argmax_host.argtypes = [fp, sz, C.POINTER(sz)]
    L.l2z_attention_decode.argtypes = [C.c_int, C.c_int, fp, fp, fp, fp] + [C.c_int] * 5
    L.l2z_option_set.argtypes = [C.c_char_p, C.c_longlong]
    L.l2z_comm_unique_id.argtypes = [vp]
    L.l2z_comm_init.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.POINTER(vp)]
    L.l2z_comm_p2p_export.argtypes = [vp, sz, vp]
    if hasattr(L, "l2z_comm_p2p_export_sized"):
        L.l2z_comm_p2p_export_sized.argtypes = [vp, sz, sz, vp]
    L.l2z_comm_p2p_connect.argtypes = [vp, vp]
    L.l2z_comm_rank.argtypes = [vp, ip, ip]
    if hasattr(L, "l2z_comm_p2p_connect_solo"):
        L.l2z_comm_p2p_connect_solo.argtypes = [vp]
    if hasattr(L, "l2z_comm_rccl_info"):
        L.l2z_comm_rccl_info.argtypes = [C.c_char_p, sz, ip]
    if hasattr(L, "l2z_runstate_form"):
        L.l2z_runstate_form.argtypes = [vp, ip]
    if hasattr(L, "l2z_comm_p2p_pingpong"):
        L.l2z_comm_p2p_pingpong.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.l2z_comm_peer_copy_probe.argtypes = [vp, C.c_int, sz, C.c_int, C.POINTER(C.c_double)]
    if hasattr(L, "l2z_comm_transports"):  # an older build loaded through L2Z_LIB (A/B runs) lacks the newer entry points
        L.l2z_comm_transports.argtypes = [vp, ip, ip]
    L.l2z_comm_free.argtypes = [vp]
    L.l2z_comm_free.restype = None
    L.l2z_comm_init_emulated.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.l2z_emu_transformer.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int]
    L.l2z_prefill_attention.argtypes = [C.c_int, fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.l2z_prefill_plan.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    L.l2z_prefill_plan_model.argtypes = [cfgp, C.c_int, C.POINTER(C.c_int), C.c_int]
    if hasattr(L, "l2z_shard_plan"):
        L.l2z_shard_plan.argtypes = [cfgp, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    L.l2z_prefill_tile.argtypes = [C.c_int, C.c_int, C.c_int]
    if hasattr(L, "l2z_prefill_cores"):
        L.l2z_prefill_cores.argtypes = [C.c_longlong, C.c_int, C.c_int]
    if hasattr(L, "l2z_prefill_gemm_plan"):
        L.l2z_prefill_gemm_plan.argtypes = [C.POINTER(GemmShape), C.POINTER(GemmPlan)]
    if hasattr(L, "l2z_prefill_split_k"):
        L.l2z_prefill_split_k.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int]
    L.l2z_emu_prefill.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int32), C.c_int, C.c_int]
    L.l2z_shard_range.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int64)]
    _lib = L
    return L


def _chk(code: int) -> None:
    if code != OK:
        raise L2ZError(code, lib().l2z_last_error().decode(errors="replace"))


def _fp(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def device_count() -> int:
    n = C.c_int(0)
    _chk(lib().l2z_device_count(C.byref(n)))
    return n.value


def device_info(dev: int = 0):
    name = C.create_string_buffer(256)
    cus, hbm = C.c_int(0), C.c_uint64(0)
    _chk(lib().l2z_device_info(dev, name, 256, C.byref(cus), C.byref(hbm)))
    return name.value.decode(), cus.value, hbm.value


def shard_range(rows: int, granule: int, rank: int, world: int):
    r0, r1 = C.c_int64(0), C.c_int64(0)
    _chk(lib().l2z_shard_range(rows, granule, rank, world, C.byref(r0), C.byref(r1)))
    return r0.value, r1.value


def _cfg(cfg) -> L2ZConfig:
    if isinstance(cfg, L2ZConfig):
        return cfg
    vals = cfg.as_i32() if hasattr(cfg, "as_i32") else cfg
    return L2ZConfig(*[int(v) for v in vals])


class Comm:
    """Multi-GPU shard group (l2z_comm_*)."""

    def __init__(self, rank: int, world: int, uid: bytes | None, device: int, emulated=False):
        self.h = C.c_void_p()
        if emulated:  # rank descriptor only (l2z_emu_transformer), no RCCL
            _chk(lib().l2z_comm_init_emulated(rank, world, device, C.byref(self.h)))
        else:
            buf = C.create_string_buffer(uid, COMM_ID_BYTES) if uid is not None else None
            _chk(lib().l2z_comm_init(rank, world, buf, device, C.byref(self.h)))
        self.rank, self.world = rank, world

    def p2p_export(self, max_vector_floats: int, max_matrix_width: int | None = None) -> bytes:
        """Allocate this rank's landing arena; returns its 64-byte IPC handle (to be all-gathered).
        max_matrix_width = max(dim, hidden_dim) sizes the sharded prefill's bulk regions."""
        buf = C.create_string_buffer(COMM_IPC_BYTES)
        if max_matrix_width is None:
            _chk(lib().l2z_comm_p2p_export(self.h, max_vector_floats, buf))
        else:
            _chk(lib().l2z_comm_p2p_export_sized(self.h, max_vector_floats, max_matrix_width, buf))
        return buf.raw

    def p2p_connect(self, handles: bytes) -> None:
        """handles: every rank's p2p_export() result concatenated in rank order."""
        assert len(handles) == COMM_IPC_BYTES * self.world
        buf = C.create_string_buffer(handles, len(handles))
        _chk(lib().l2z_comm_p2p_connect(self.h, buf))

    def p2p_connect_solo(self) -> None:
        """Measurement: this rank alone, peers' arenas a local sink, no wait ever blocks (l2z_comm_p2p_connect_solo)."""
        _chk(lib().l2z_comm_p2p_connect_solo(self.h))

    def p2p_pingpong(self, other: int, initiator: bool, iters: int = 2000) -> float:
        """microseconds per round trip of one LL word each way between this rank and `other` (both ranks call)"""
        v = C.c_double(0)
        _chk(lib().l2z_comm_p2p_pingpong(self.h, other, 1 if initiator else 0, iters, C.byref(v)))
        return v.value

    def peer_copy_probe(self, other: int, nbytes: int = 16384, iters: int = 200) -> float:
        """microseconds per synchronised device-to-device copy of `nbytes` into rank `other`'s arena (one rank calls)"""
        v = C.c_double(0)
        _chk(lib().l2z_comm_peer_copy_probe(self.h, other, nbytes, iters, C.byref(v)))
        return v.value

    def transports(self) -> dict:
        """{"rccl_ranks": ranks RCCL reports for the communicator (0: none), "p2p": arenas connected}"""
        n, p = C.c_int(0), C.c_int(0)
        _chk(lib().l2z_comm_transports(self.h, C.byref(n), C.byref(p)))
        return {"rccl_ranks": n.value, "p2p": bool(p.value)}

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _chk(lib().l2z_comm_unique_id(buf))
        return buf.raw

    def close(self):
        if self.h:
            lib().l2z_comm_free(self.h)
            self.h = C.c_void_p()


class Weights:
    """src/main.zig:53 Weights, device resident."""

    def __init__(self, cfg, blob: np.ndarray | None, shared: bool, *, seed: int | None = None,
                 comm: Comm | None = None):
        self.cfg = _cfg(cfg)
        self.h = C.c_void_p()
        ch = comm.h if comm is not None else None
        if blob is not None:
            b = blob if (blob.dtype == np.float32 and blob.flags["C_CONTIGUOUS"]) else _f32(blob)
            _chk(lib().l2z_weights_init(C.byref(self.cfg), _fp(b), b.size, int(shared), ch,
                                        C.byref(self.h)))
        else:
            assert seed is not None
            _chk(lib().l2z_weights_init_synthetic(C.byref(self.cfg), int(shared), seed, ch,
                                                  C.byref(self.h)))

    @classmethod
    def from_q8(cls, cfg, body, shared: bool, gs: int, *, comm: Comm | None = None) -> "Weights":
        """int8 group-quantized weights from the body of a llama2.c version-2 checkpoint (the file from byte 256 on:
        checkpoint.read_checkpoint_v2).  Only the single-sequence decode takes them (l2z_weights_init_q8)."""
        self = cls.__new__(cls)
        self.cfg = _cfg(cfg)
        self.h = C.c_void_p()
        self.gs = int(gs)
        b = np.ascontiguousarray(np.asarray(body).view(np.uint8).reshape(-1))
        _chk(lib().l2z_weights_init_q8(C.byref(self.cfg), b.ctypes.data_as(C.c_void_p), b.size, int(shared), int(gs),
                                       comm.h if comm is not None else None, C.byref(self.h)))
        return self

    @classmethod
    def quantized(cls, w_f32: "Weights", gs: int) -> "Weights":
        """w_f32 (unsharded f32 weights) quantized ON THE DEVICE by the weight rule; independent of w_f32 afterwards."""
        self = cls.__new__(cls)
        self.cfg = w_f32.cfg
        self.h = C.c_void_p()
        self.gs = int(gs)
        _chk(lib().l2z_weights_init_q8_from(w_f32.h, int(gs), C.byref(self.h)))
        return self

    def q8_read(self, name: str, layer: int = 0):
        """(q int8 [rows, cols], s f32 [rows, cols // gs]) of one layer of a quantized tensor, in the file's row order."""
        c = self.cfg
        kvd = c.dim // c.n_heads * c.n_kv_heads
        rows, cols = {"token_embedding_table": (c.vocab_size, c.dim), "wcls": (c.vocab_size, c.dim), "wq": (c.dim, c.dim),
                      "wk": (kvd, c.dim), "wv": (kvd, c.dim), "wo": (c.dim, c.dim), "w1": (c.hidden_dim, c.dim),
                      "w2": (c.dim, c.hidden_dim), "w3": (c.hidden_dim, c.dim)}[name]
        q = np.empty((rows, cols), np.int8)
        s = np.empty((rows, cols // self.gs), np.float32)
        _chk(lib().l2z_weights_q8_read(self.h, name.encode(), layer, q.ctypes.data_as(C.POINTER(C.c_int8)), _fp(s)))
        return q, s

    def read(self, offset: int, count: int) -> np.ndarray:
        out = np.empty(count, np.float32)
        _chk(lib().l2z_weights_read(self.h, offset, count, _fp(out)))
        return out

    def close(self):
        if self.h:
            lib().l2z_weights_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


KV_PAGE = 64  # L2Z_KV_PAGE


class KvPool:
    """l2z_kvpool: n_pages pages of KV_PAGE positions that paged runstates (RunState(cfg, pool=pool)) draw from on demand
    (a preview surface of the test library: include/llama2_hip_test.h)."""

    def __init__(self, cfg, n_pages: int):
        self.cfg = _cfg(cfg)
        self.h = C.c_void_p()
        _chk(lib().l2z_kvpool_init(C.byref(self.cfg), int(n_pages), C.byref(self.h)))

    def info(self) -> dict:
        n, f, b = C.c_int(0), C.c_int(0), C.c_uint64(0)
        _chk(lib().l2z_kvpool_info(self.h, C.byref(n), C.byref(f), C.byref(b)))
        return {"n_pages": n.value, "n_free": f.value, "page_bytes": b.value}

    def close(self):
        """Raises L2ZError (ERR_STATE) while a runstate made from the pool is alive; the pool then stays usable."""
        if self.h:
            _chk(lib().l2z_kvpool_free(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RunState:
    """src/main.zig:119 RunState, device resident.  pool: a paged runstate (l2z_runstate_init_paged), which holds no KV
    caches of its own and is taken by the wide family only."""

    def __init__(self, cfg, comm: Comm | None = None, pool: KvPool | None = None):
        self.cfg = _cfg(cfg)
        self.h = C.c_void_p()
        self.pool = pool   # (kept alive: the pool outlives its runstates)
        if pool is not None:
            assert comm is None, "a paged runstate is unsharded"
            _chk(lib().l2z_runstate_init_paged(C.byref(self.cfg), pool.h, C.byref(self.h)))
            return
        _chk(lib().l2z_runstate_init(C.byref(self.cfg), comm.h if comm is not None else None,
                                     C.byref(self.h)))

    def pages(self) -> np.ndarray:
        """l2z_runstate_pages: the page table, one pool page id per KV_PAGE positions of seq_len, -1 where none is attached."""
        cap = (self.cfg.seq_len + KV_PAGE - 1) // KV_PAGE
        ids = np.full(max(cap, 1), -1, np.int32)
        n = C.c_int(0)
        _chk(lib().l2z_runstate_pages(self.h, C.byref(n), ids.ctypes.data_as(C.POINTER(C.c_int32)), cap))
        return ids[:cap].copy()

    def trim(self, n_pos: int) -> None:
        """l2z_runstate_trim: give back every page that lies wholly at or above n_pos."""
        _chk(lib().l2z_runstate_trim(self.h, int(n_pos)))

    def transformer(self, token: int, pos: int, w: Weights) -> None:
        """src/main.zig:285"""
        _chk(lib().l2z_transformer(token, pos, C.byref(self.cfg), self.h, w.h))

    def prefill(self, tokens, pos0: int, w: Weights) -> None:
        """l2z_prefill: the state change of transformer(tokens[i], pos0+i) for all i, batched."""
        t = np.ascontiguousarray(tokens, np.int32)
        _chk(lib().l2z_prefill(t.ctypes.data_as(C.POINTER(C.c_int32)), t.size, pos0,
                               C.byref(self.cfg), self.h, w.h))

    def prefill_q8(self, tokens, pos0: int, w: Weights) -> None:
        """l2z_prefill_q8 (a preview entry point of the test library): prefill's state change on int8 group-quantized
        weights, on the int8 matrix cores; agrees with the stepped pass up to f32 summation order."""
        t = np.ascontiguousarray(tokens, np.int32)
        _chk(lib().l2z_prefill_q8(t.ctypes.data_as(C.POINTER(C.c_int32)), t.size, pos0, C.byref(self.cfg), self.h, w.h))

    def score(self, tokens, pos0: int, w: Weights, targets=None, top1: bool = True):
        """l2z_score: prefill(tokens, pos0) plus, per position, (log-prob of its target, top-1 token id) as two arrays.
        targets=None: the next token of each position, none (-1, log-prob 0) for the last; top1=False: no top-1 (None)."""
        t = np.ascontiguousarray(tokens, np.int32)
        if targets is None:
            tg = np.append(t[1:], np.int32(-1)).astype(np.int32)
        else:
            tg = np.ascontiguousarray(targets, np.int32)
            assert tg.size == t.size
        lp = np.zeros(t.size, np.float32)
        tp = np.zeros(t.size, np.int32) if top1 else None
        i32p = C.POINTER(C.c_int32)
        _chk(lib().l2z_score(t.ctypes.data_as(i32p), t.size, pos0, tg.ctypes.data_as(i32p), C.byref(self.cfg), self.h, w.h,
                             _fp(lp), tp.ctypes.data_as(i32p) if top1 else None))
        return lp, tp

    def score_slab_set(self, slab_cols: int) -> None:
        """l2z_score_slab_set (test hook): vocabulary rows per slab of score()'s classifier product, 0: the default."""
        _chk(lib().l2z_score_slab_set(self.h, slab_cols))

    def _verify_call(self, name: str, tokens, pos0: int, w: Weights, draw=None, iters=None):
        """One call of the chain verify family: lib().<name>(tokens, n, pos0, [temperature, top_p, coins,] config, runstate,
        weights, ...) with draw = (temperature, top_p, coins) where the entry point takes a draw, and behind them next and
        accepted -> (next: int32[n], accepted), or -- iters -- iters and the time -> milliseconds per pass."""
        t = np.ascontiguousarray(tokens, np.int32)
        i32p = C.POINTER(C.c_int32)
        args = [t.ctypes.data_as(i32p), t.size, pos0]
        if draw is not None:
            temperature, top_p, coins = draw
            c = None if coins is None else np.ascontiguousarray(coins, np.float32)
            if c is not None and c.size < t.size:
                raise ValueError(f"{c.size} coins for {t.size} rows")
            args += [C.c_float(temperature), C.c_float(top_p), None if c is None else _fp(c)]
        args += [C.byref(self.cfg), self.h, w.h]
        if iters is not None:
            ms = C.c_double(0.0)
            _chk(getattr(lib(), name)(*args, iters, C.byref(ms)))
            return ms.value
        nxt = np.zeros(max(t.size, 1), np.int32)
        a = C.c_int(0)
        _chk(getattr(lib(), name)(*args, nxt.ctypes.data_as(i32p), C.byref(a)))
        return nxt[: t.size].copy(), a.value

    def verify(self, tokens, pos0: int, w: Weights):
        """l2z_verify: tokens[0] is the sequence's token at pos0, tokens[1:] are guesses for the positions after it.
        Returns (next: int32[n], accepted): next[i] = the model's argmax after tokens[:i + 1]; next[:accepted + 1] are
        the sequence's next tokens and the runstate stands at pos0 + accepted + 1 with the logits behind next[accepted]."""
        return self._verify_call("l2z_verify", tokens, pos0, w)

    def verify_logits(self, row: int) -> np.ndarray:
        """l2z_verify_logits_read (test hook): row `row` of the last verify() call's logits matrix."""
        out = np.empty(self.cfg.vocab_size, np.float32)
        _chk(lib().l2z_verify_logits_read(self.h, row, _fp(out)))
        return out

    def verify_time(self, tokens, pos0: int, w: Weights, iters: int) -> float:
        """l2z_verify_time: milliseconds per verify pass, device events over `iters` passes (after one untimed)."""
        return self._verify_call("l2z_verify_time", tokens, pos0, w, None, iters)

    def verify_sample(self, tokens, pos0: int, w: Weights, temperature: float, top_p: float, coins):
        """l2z_verify_sample: verify() with next[i] drawn as sample_batch draws it from row i's logits with
        (temperature, top_p, coins[i]); coins[i] is the coin of position pos0 + i (None: NULL, for temperature 0).
        Returns (next: int32[n], accepted) as verify()."""
        return self._verify_call("l2z_verify_sample", tokens, pos0, w, (temperature, top_p, coins))

    def verify_sample_time(self, tokens, pos0: int, w: Weights, temperature: float, top_p: float, coins, iters: int) -> float:
        """l2z_verify_sample_time: milliseconds per sampled verify pass, device events over `iters` passes."""
        return self._verify_call("l2z_verify_sample_time", tokens, pos0, w, (temperature, top_p, coins), iters)

    def verify_q8(self, tokens, pos0: int, w: Weights, temperature: float = 0.0, top_p: float = 1.0, coins=None):
        """l2z_verify_q8 (a preview entry point of the test library): verify() on int8 group-quantized weights, or -- with a
        temperature -- verify_sample(), coins[i] the coin of position pos0 + i.  Returns (next: int32[n], accepted)."""
        return self._verify_call("l2z_verify_q8", tokens, pos0, w, (temperature, top_p, coins))

    def verify_q8_time(self, tokens, pos0: int, w: Weights, iters: int, temperature: float = 0.0, top_p: float = 1.0,
                       coins=None) -> float:
        """l2z_verify_q8_time: milliseconds per verify_q8 pass, device events over `iters` passes (after one untimed)."""
        return self._verify_call("l2z_verify_q8_time", tokens, pos0, w, (temperature, top_p, coins), iters)

    def verify_tree(self, tokens, parent, pos0: int, w: Weights, temperature: float = 0.0, top_p: float = 1.0, coins=None):
        """l2z_verify_tree (a preview entry point of the test library: include/llama2_hip_test.h): verify() for a TREE of
        guesses.  tokens[0] is the sequence's token at pos0 with parent[0] == -1; node i > 0 is a guess behind node
        parent[i] < i and stands for position pos0 + depth_i.  coins[d] is the coin of position pos0 + d (one per DEPTH;
        None at temperature 0).  Returns (next: int32[n], path: int32[accepted + 1], accepted): next[i] = the model's id
        after the tokens on the path root -> i, path = the nodes the verdict walked from the root; the sequence's next
        tokens are next[path] and the runstate stands at pos0 + accepted + 1 with the logits behind next[path[-1]]."""
        t = np.ascontiguousarray(tokens, np.int32).reshape(-1)
        par = np.ascontiguousarray(parent, np.int32).reshape(-1)
        if par.size != t.size:
            raise ValueError(f"{par.size} parents for {t.size} nodes")
        c = None if coins is None else np.ascontiguousarray(coins, np.float32).reshape(-1)
        tb, pb = np.zeros(max(t.size, 1), np.int32), np.zeros(max(t.size, 1), np.int32)
        tb[: t.size], pb[: t.size] = t, par
        nxt, path = np.zeros(max(t.size, 1), np.int32), np.zeros(max(t.size, 1), np.int32)
        a = C.c_int(0)
        i32p = C.POINTER(C.c_int32)
        _chk(lib().l2z_verify_tree(tb.ctypes.data_as(i32p), pb.ctypes.data_as(i32p), t.size, pos0, C.c_float(temperature),
                                   C.c_float(top_p), None if c is None else _fp(c), C.byref(self.cfg), self.h, w.h,
                                   nxt.ctypes.data_as(i32p), path.ctypes.data_as(i32p), C.byref(a)))
        return nxt[: t.size].copy(), path[: a.value + 1].copy(), a.value

    def verify_tree_time(self, tokens, parent, pos0: int, w: Weights, iters: int, temperature: float = 0.0,
                         top_p: float = 1.0, coins=None) -> float:
        """l2z_verify_tree_time: milliseconds per tree verify pass, device events over `iters` passes (after one untimed)."""
        t = np.ascontiguousarray(tokens, np.int32).reshape(-1)
        par = np.ascontiguousarray(parent, np.int32).reshape(-1)
        c = None if coins is None else np.ascontiguousarray(coins, np.float32).reshape(-1)
        ms = C.c_double(0.0)
        i32p = C.POINTER(C.c_int32)
        _chk(lib().l2z_verify_tree_time(t.ctypes.data_as(i32p), par.ctypes.data_as(i32p), t.size, pos0, C.c_float(temperature),
                                        C.c_float(top_p), None if c is None else _fp(c), C.byref(self.cfg), self.h, w.h,
                                        iters, C.byref(ms)))
        return ms.value

    def argmax(self) -> int:
        t = C.c_int(0)
        _chk(lib().l2z_argmax(self.h, C.byref(t)))
        return t.value

    def logits(self) -> np.ndarray:
        out = np.empty(self.cfg.vocab_size, np.float32)
        _chk(lib().l2z_logits_read(self.h, _fp(out)))
        return out

    def probs(self, temperature: float = 1.0) -> np.ndarray:
        """softmax(logits / temperature) computed on the device (l2z_probs_read)."""
        out = np.empty(self.cfg.vocab_size, np.float32)
        _chk(lib().l2z_probs_read(self.h, C.c_float(temperature), _fp(out)))
        return out

    def write_logits(self, logits) -> None:
        """l2z_logits_write (test hook): place exact logits in the runstate."""
        lg = _f32(logits)
        assert lg.size == self.cfg.vocab_size
        _chk(lib().l2z_logits_write(self.h, _fp(lg)))

    def read(self, name: str, offset: int, count: int) -> np.ndarray:
        out = np.empty(count, np.float32)
        _chk(lib().l2z_runstate_read(self.h, name.encode(), offset, count, _fp(out)))
        return out

    def greedy_begin(self, prompt=()) -> None:
        p = np.ascontiguousarray(prompt, np.int32)
        _chk(lib().l2z_greedy_begin(self.h, p.ctypes.data_as(C.POINTER(C.c_int32)), p.size))

    def greedy_run(self, w: Weights, n_steps: int) -> np.ndarray:
        out = np.zeros(max(n_steps, 1), np.int32)
        n = C.c_int(0)
        _chk(lib().l2z_greedy_run(C.byref(self.cfg), self.h, w.h, n_steps,
                                  out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)))
        return out[: n.value].copy()

    def sample_run(self, w: Weights, n_steps: int, temperature: float, top_p: float, coins=None) -> np.ndarray:
        """l2z_sample_run (a preview entry point of the test library: include/llama2_hip_test.h): greedy_run with every
        generated token DRAWN on the device, after greedy_begin.  coins[i] is the coin of the call's step i (unused at a
        prompt step); None at temperature 0.  Returns the ids of the steps that ran."""
        out = np.zeros(max(n_steps, 1), np.int32)
        n = C.c_int(0)
        cp = None
        if coins is not None:
            coins = np.ascontiguousarray(coins, np.float32).reshape(-1)
            if coins.size < n_steps:
                raise ValueError(f"{coins.size} coins for {n_steps} steps")
            cp = _fp(coins)
        _chk(lib().l2z_sample_run(C.byref(self.cfg), self.h, w.h, n_steps, C.c_float(temperature), C.c_float(top_p), cp,
                                  out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)))
        return out[: n.value].copy()

    def profile_forward(self, token: int, pos: int, w: Weights):
        ms = (C.c_double * len(KINDS))()
        cnt = (C.c_int * len(KINDS))()
        _chk(lib().l2z_profile_forward(token, pos, C.byref(self.cfg), self.h, w.h, ms, cnt,
                                       len(KINDS)))
        return {k: (ms[i], cnt[i]) for i, k in enumerate(KINDS)}

    def form(self) -> int:
        """The decode structure this state runs: bit 0 paired mat-vec blocks, bit 1 two chains, bit 2 persistent launches."""
        f = C.c_int(0)
        _chk(lib().l2z_runstate_form(self.h, C.byref(f)))
        return f.value

    def time_kind(self, kind: str, pos: int, w: Weights, reps: int = 4):
        """(average ms per launch, launches) of one kind of launch, back to back between one event pair."""
        ms, n = C.c_double(0), C.c_int(0)
        _chk(lib().l2z_time_kind(KINDS.index(kind), pos, C.byref(self.cfg), self.h, w.h, reps, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def stream_read_probe(self, w: Weights, slice_bytes: int = 0, reps: int = 8):
        """(average, best) GB/s of a pure streaming-read kernel over the resident weight blob."""
        avg, best = C.c_double(0), C.c_double(0)
        _chk(lib().l2z_stream_read_probe(self.h, w.h, slice_bytes, reps, C.byref(avg), C.byref(best)))
        return avg.value, best.value

    def d2d_copy_probe(self, w: Weights, slice_bytes: int = 0, reps: int = 8):
        """(average, best) GB/s of bytes copied by a device-to-device hipMemcpyAsync of pieces of the weight blob."""
        avg, best = C.c_double(0), C.c_double(0)
        _chk(lib().l2z_d2d_copy_probe(self.h, w.h, slice_bytes, reps, C.byref(avg), C.byref(best)))
        return avg.value, best.value

    def synchronize(self) -> None:
        _chk(lib().l2z_synchronize(self.h))

    def close(self):
        if self.h:
            lib().l2z_runstate_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


BATCH_MAX = 16  # L2Z_BATCH_MAX


def _batch_args(states, tokens, pos):
    n = len(states)
    ss = (C.c_void_p * max(n, 1))(*[s.h for s in states])
    t = np.ascontiguousarray(tokens, np.int32)
    p = np.ascontiguousarray(pos, np.int32)
    return n, ss, t, p


def _batch_call(name: str, states, tokens, pos, w: Weights, iters=None):
    """lib().<name>(n, tokens, pos, config, states, weights), or -- iters -- with iters and the time behind them ->
    milliseconds per step.  The config is states[0]'s."""
    n, ss, t, p = _batch_args(states, tokens, pos)
    i32p = C.POINTER(C.c_int32)
    args = (n, t.ctypes.data_as(i32p), p.ctypes.data_as(i32p), C.byref(states[0].cfg if n else L2ZConfig()), ss, w.h)
    if iters is None:
        return _chk(getattr(lib(), name)(*args))
    ms = C.c_double(0.0)
    _chk(getattr(lib(), name)(*args, iters, C.byref(ms)))
    return ms.value


def transformer_batch(states, tokens, pos, w: Weights) -> None:
    """l2z_transformer_batch: transformer(tokens[i], pos[i]) on states[i] for every i, one sweep of the weights.
    The config is states[0]'s (the call checks that every runstate and the weights share it)."""
    _batch_call("l2z_transformer_batch", states, tokens, pos, w)


def argmax_batch(states) -> np.ndarray:
    """l2z_argmax_batch: the argmax of every runstate's logits, one launch."""
    n = len(states)
    ss = (C.c_void_p * max(n, 1))(*[s.h for s in states])
    out = np.zeros(max(n, 1), np.int32)
    _chk(lib().l2z_argmax_batch(n, ss, out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out[:n].copy()


def batch_time(states, tokens, pos, w: Weights, iters: int) -> float:
    """l2z_batch_time: milliseconds per batched step, device events over `iters` steps (after one untimed)."""
    return _batch_call("l2z_batch_time", states, tokens, pos, w, iters)


def transformer_batch_q8(states, tokens, pos, w: Weights) -> None:
    """l2z_transformer_batch_q8 (a preview entry point of the test library): transformer_batch on int8 group-quantized
    weights; argmax_batch and sample_batch work behind it."""
    _batch_call("l2z_transformer_batch_q8", states, tokens, pos, w)


def batch_q8_time(states, tokens, pos, w: Weights, iters: int) -> float:
    """l2z_batch_q8_time: milliseconds per transformer_batch_q8 step, device events over `iters` steps (after one untimed)."""
    return _batch_call("l2z_batch_q8_time", states, tokens, pos, w, iters)


def _sample_args(states, temperature, top_p, coins):
    n = len(states)
    ss = (C.c_void_p * max(n, 1))(*[s.h for s in states])
    vals = []
    for v in (temperature, top_p, coins):
        a = np.zeros(max(n, 1), np.float32)
        a[:n] = np.broadcast_to(np.asarray(v, np.float32), (n,)) if n else []
        vals.append(a)
    return n, ss, vals


def sample_batch(states, temperature, top_p, coins) -> np.ndarray:
    """l2z_sample_batch: one token per runstate, drawn on the device from its logits with temperature[i], top_p[i] and
    the number coins[i] exactly as the host samplers draw (scalars apply to every row)."""
    n, ss, (t, p, c) = _sample_args(states, temperature, top_p, coins)
    out = np.zeros(max(n, 1), np.int32)
    _chk(lib().l2z_sample_batch(n, ss, _fp(t), _fp(p), _fp(c), out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out[:n].copy()


def sample_time(states, temperature, top_p, coins, iters: int) -> float:
    """l2z_sample_time: milliseconds per l2z_sample_batch launch, device events over `iters` launches."""
    n, ss, (t, p, c) = _sample_args(states, temperature, top_p, coins)
    ms = C.c_double(0.0)
    _chk(lib().l2z_sample_time(n, ss, _fp(t), _fp(p), _fp(c), iters, C.byref(ms)))
    return ms.value


def prefill_batch(states, token_lists, pos0s, w: Weights) -> None:
    """l2z_prefill_batch: prefill(token_lists[j], pos0s[j]) on states[j] for every j, ONE pass over the concatenated rows
    (a preview entry point of the test library: include/llama2_hip_test.h).  pos0s: one int per sequence, or a scalar."""
    n = len(states)
    ss = (C.c_void_p * max(n, 1))(*[s.h for s in states])
    lists = [np.ascontiguousarray(t, np.int32).reshape(-1) for t in token_lists]
    assert len(lists) == n, "one token list per runstate"
    nt = np.zeros(max(n, 1), np.int32)
    nt[:n] = [t.size for t in lists]
    p0 = np.zeros(max(n, 1), np.int32)
    p0[:n] = np.broadcast_to(np.asarray(pos0s, np.int32), (n,)) if n else []
    t = np.ascontiguousarray(np.concatenate(lists + [np.zeros(1, np.int32)]), np.int32)  # (never empty)
    cfg = states[0].cfg if n else L2ZConfig()
    i32p = C.POINTER(C.c_int32)
    _chk(lib().l2z_prefill_batch(n, t.ctypes.data_as(i32p), nt.ctypes.data_as(i32p), p0.ctypes.data_as(i32p),
                                 C.byref(cfg), ss, w.h))


WIDE_MAX = 128  # L2Z_WIDE_MAX


def transformer_wide(states, tokens, pos, w: Weights, want_next: bool = True):
    """l2z_transformer_wide: transformer(tokens[i], pos[i]) on states[i] for every i of up to WIDE_MAX runstates, one sweep
    of the weights on the matrix cores (a preview entry point of the test library: include/llama2_hip_test.h).
    want_next: returns every row's argmax (taken on the device; the call is synchronous); otherwise None, and the call is
    asynchronous as transformer_batch is."""
    n, ss, t, p = _batch_args(states, tokens, pos)
    cfg = states[0].cfg if n else L2ZConfig()
    i32p = C.POINTER(C.c_int32)
    nxt = np.zeros(max(n, 1), np.int32) if want_next else None
    _chk(lib().l2z_transformer_wide(n, t.ctypes.data_as(i32p), p.ctypes.data_as(i32p), C.byref(cfg), ss, w.h,
                                    nxt.ctypes.data_as(i32p) if want_next else None))
    return nxt[:n].copy() if want_next else None


def generate_wide(states, first_tokens, pos0s, w: Weights, n_steps: int) -> np.ndarray:
    """The greedy loop over transformer_wide: states[i] is fed first_tokens[i] at pos0s[i], then its own argmax, for n_steps
    steps -- one call per step, no host argmax.  Returns the ids [n_steps, n] (row k = the tokens step k chose)."""
    n = len(states)
    tok = np.array(np.broadcast_to(np.asarray(first_tokens, np.int32), (n,)), np.int32)
    pos = np.array(np.broadcast_to(np.asarray(pos0s, np.int32), (n,)), np.int32)
    out = np.zeros((n_steps, n), np.int32)
    for k in range(n_steps):
        tok = transformer_wide(states, tok, pos + k, w)
        out[k] = tok
    return out


def wide_run(states, first_tokens, pos0s, w: Weights, n_steps: int, temperature=None, top_p=None, coins=None) -> np.ndarray:
    """l2z_wide_run: n_steps transformer_wide steps of the same runstates in ONE call, every row's token drawn on the device
    as sample_batch draws it and fed to the next step there (a preview entry point of the test library:
    include/llama2_hip_test.h).  states[i] is fed first_tokens[i] at pos0s[i].  temperature=None: every row takes its
    argmax; otherwise temperature and top_p are one value per row (or a scalar for all) and coins is [n_steps, n] (or a
    scalar, or one row per step broadcast over the rows; None where every temperature is 0).
    Returns the ids [n_steps, n] (row k = the tokens step k drew), bit for bit those of the loop of transformer_wide and
    sample_batch calls."""
    n = len(states)
    ss = (C.c_void_p * max(n, 1))(*[s.h for s in states])
    steps = max(int(n_steps), 0)

    def per_row(v, dtype):
        a = np.zeros(max(n, 1), dtype)
        a[:n] = np.broadcast_to(np.asarray(v, dtype), (n,)) if n else []
        return a
    tok, pos = per_row(first_tokens, np.int32), per_row(pos0s, np.int32)
    t = p = c = None
    if temperature is not None:
        t = per_row(temperature, np.float32)
        p = per_row(top_p, np.float32) if top_p is not None else None
        if coins is not None:
            c = np.zeros((max(steps, 1), max(n, 1)), np.float32)
            c[:steps, :n] = np.broadcast_to(np.asarray(coins, np.float32), (steps, n))
    out = np.zeros((max(steps, 1), max(n, 1)), np.int32)
    cfg = states[0].cfg if n else L2ZConfig()
    i32p = C.POINTER(C.c_int32)
    _chk(lib().l2z_wide_run(n, tok.ctypes.data_as(i32p), pos.ctypes.data_as(i32p), int(n_steps),
                            _fp(t) if t is not None else None, _fp(p) if p is not None else None,
                            _fp(c) if c is not None else None, C.byref(cfg), ss, w.h, out.ctypes.data_as(i32p)))
    return out[:steps, :n].copy()   # (n >= 1 here: the rows are n wide, as the call wrote them)


def generate_wide_sample(states, first_tokens, pos0s, w: Weights, n_steps: int, temperature=None, top_p=None, coins=None,
                         bos: int = 1):
    """The convenience loop over wide_run: one call, then every column cut after its first BOS (main.zig:1038-1040; the
    device stops no row, what a row drew after its BOS is discarded here).  Returns a list of n int32 arrays, sequence
    i's tokens up to and including its BOS if it drew one."""
    ids = wide_run(states, first_tokens, pos0s, w, n_steps, temperature, top_p, coins)
    out = []
    for i in range(ids.shape[1]):
        col = ids[:, i]
        hit = np.flatnonzero(col == bos)
        out.append(col[:hit[0] + 1].copy() if hit.size else col.copy())
    return out


def verify_batch(states, token_lists, pos0s, w: Weights, temperature=None, top_p=None, coin_lists=None):
    """l2z_verify_batch: RunState.verify(token_lists[j], pos0s[j]) on states[j] for every j in ONE sweep of the weights, bit
    for bit (a preview entry point of the test library: include/llama2_hip_test.h).  temperature=None: greedy; otherwise
    temperature and top_p are one value per sequence (or a scalar for all) and coin_lists[j] holds a coin per row of
    sequence j (None, or a None entry, where the temperature is 0): RunState.verify_sample per sequence.
    Returns (list of next arrays, accepted array).  states[0].verify_logits(r) then reads concatenated row r."""
    return _verify_rows(lib().l2z_verify_batch, states, token_lists, pos0s, w, temperature, top_p, coin_lists)


def verify_wide(states, token_lists, pos0s, w: Weights, temperature=None, top_p=None, coin_lists=None):
    """l2z_verify_wide: verify_batch's call for up to WIDE_MAX rows in all (each sequence up to BATCH_MAX) in ONE sweep of the
    weights on the matrix cores (a preview entry point of the test library: include/llama2_hip_test.h).  The arguments and
    the return are verify_batch's; the values agree with RunState.verify's at the fp32 parity bar, not bit for bit."""
    return _verify_rows(lib().l2z_verify_wide, states, token_lists, pos0s, w, temperature, top_p, coin_lists)


def _verify_rows(call, states, token_lists, pos0s, w, temperature, top_p, coin_lists):
    """the arguments l2z_verify_batch and l2z_verify_wide share, the call, and its outputs cut per sequence"""
    n = len(states)
    ss = (C.c_void_p * max(n, 1))(*[s.h for s in states])
    lists = [np.ascontiguousarray(t, np.int32).reshape(-1) for t in token_lists]
    assert len(lists) == n, "one token list per runstate"
    nt = np.zeros(max(n, 1), np.int32)
    nt[:n] = [t.size for t in lists]
    p0 = np.zeros(max(n, 1), np.int32)
    p0[:n] = np.broadcast_to(np.asarray(pos0s, np.int32), (n,)) if n else []
    t = np.ascontiguousarray(np.concatenate(lists + [np.zeros(1, np.int32)]), np.int32)  # (never empty)
    rows = int(nt[:n].sum())
    tp = pp = cp = None
    if temperature is not None:
        tp, pp = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
        tp[:n] = np.broadcast_to(np.asarray(temperature, np.float32), (n,)) if n else []
        pp[:n] = np.broadcast_to(np.asarray(1.0 if top_p is None else top_p, np.float32), (n,)) if n else []
        if coin_lists is not None:
            assert len(coin_lists) == n, "one coin list per runstate"
            cp = np.zeros(rows + 1, np.float32)
            r = 0
            for j, c in enumerate(coin_lists):
                if c is not None:
                    c = np.ascontiguousarray(c, np.float32).reshape(-1)
                    if c.size < lists[j].size:
                        raise ValueError(f"sequence {j}: {c.size} coins for {lists[j].size} rows")
                    cp[r: r + lists[j].size] = c[: lists[j].size]
                elif tp[j] > 0:
                    raise ValueError(f"sequence {j}: no coins at temperature {tp[j]}")
                r += lists[j].size
    nxt = np.zeros(rows + 1, np.int32)
    acc = np.zeros(max(n, 1), np.int32)
    cfg = states[0].cfg if n else L2ZConfig()
    i32p = C.POINTER(C.c_int32)
    _chk(call(n, t.ctypes.data_as(i32p), nt.ctypes.data_as(i32p), p0.ctypes.data_as(i32p),
              None if tp is None else _fp(tp), None if pp is None else _fp(pp),
              None if cp is None else _fp(cp), C.byref(cfg), ss, w.h, nxt.ctypes.data_as(i32p),
              acc.ctypes.data_as(i32p)))
    ends = np.cumsum(nt[:n])
    return [nxt[e - m: e].copy() for e, m in zip(ends, nt[:n])], acc[:n].copy()


MIXED_ROWS_MAX = 512  # L2Z_MIXED_ROWS_MAX


def step_mixed(states, token_lists, pos0s, w: Weights, temperature=None, top_p=None, coins=None) -> np.ndarray:
    """l2z_step_mixed: states[j] runs token_lists[j] at positions pos0s[j] .. in ONE sweep of the weights -- a list of one
    token is a decode step, a longer one a prompt chunk (a preview entry point of the test library:
    include/llama2_hip_test.h).  Up to WIDE_MAX sequences and MIXED_ROWS_MAX rows in all.  temperature=None: greedy;
    otherwise temperature and top_p are one value per sequence (or a scalar for all) and coins holds ONE coin per sequence
    (None where every temperature is 0).  Returns the n ids drawn from the sequences' last rows; every runstate's logits
    are its last row's."""
    n = len(states)
    ss = (C.c_void_p * max(n, 1))(*[s.h for s in states])
    lists = [np.ascontiguousarray(t, np.int32).reshape(-1) for t in token_lists]
    assert len(lists) == n, "one token list per runstate"
    nt = np.zeros(max(n, 1), np.int32)
    nt[:n] = [t.size for t in lists]
    p0 = np.zeros(max(n, 1), np.int32)
    p0[:n] = np.broadcast_to(np.asarray(pos0s, np.int32), (n,)) if n else []
    t = np.ascontiguousarray(np.concatenate(lists + [np.zeros(1, np.int32)]), np.int32)  # (never empty)
    tp = pp = cp = None
    if temperature is not None:
        tp, pp = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
        tp[:n] = np.broadcast_to(np.asarray(temperature, np.float32), (n,)) if n else []
        pp[:n] = np.broadcast_to(np.asarray(1.0 if top_p is None else top_p, np.float32), (n,)) if n else []
        if coins is not None:
            cp = np.zeros(max(n, 1), np.float32)
            cp[:n] = np.broadcast_to(np.asarray(coins, np.float32), (n,)) if n else []
    nxt = np.zeros(max(n, 1), np.int32)
    cfg = states[0].cfg if n else L2ZConfig()
    i32p = C.POINTER(C.c_int32)
    _chk(lib().l2z_step_mixed(n, t.ctypes.data_as(i32p), nt.ctypes.data_as(i32p), p0.ctypes.data_as(i32p),
                              None if tp is None else _fp(tp), None if pp is None else _fp(pp),
                              None if cp is None else _fp(cp), C.byref(cfg), ss, w.h, nxt.ctypes.data_as(i32p)))
    return nxt[:n].copy()


def serve(requests, w: Weights, pool: KvPool, *, max_seqs: int = WIDE_MAX, row_budget: int = MIXED_ROWS_MAX,
          chunk: int | None = None, temperature=None, top_p=None, coins=None, bos: int = 1):
    """Continuous batching over paged runstates: a queue of requests turned into step_mixed calls.  requests[i] =
    (tokens, max_new): the tokens fed from position 0 on (the caller's BOS included) and how many ids to draw at most.
    Every step gives each sequence that is decoding its one row, then fills what is left of row_budget with slices (of at
    most `chunk` rows; None: whatever fits) of partly prefilled or waiting requests in arrival order.  A waiting request is
    admitted only while fewer than max_seqs are in flight -- fewer than row_budget too: every sequence in flight may need a
    row of every step, so no step runs more than row_budget rows -- and the pool's free pages, less what the requests in
    flight may still take, hold its whole prompt plus max_new; nothing is preempted.  A sequence retires at `bos`, at max_new ids, or
    at seq_len; its pages go back (trim) and its runstate serves the next request.
    temperature / top_p: None (greedy), a scalar, or one value per request; coins: per request, the coin of its g-th id
    (generate_sample's convention; None where greedy).
    Returns (ids, trace): ids[i] = request i's ids (its BOS, if drawn, the last), trace[k] = step k's layout: a dict of
    "ids" (the requests, in call order), "n_tokens", "pos0" and "pages" (the pool pages each of them holds after the step,
    as RunState.pages() lists them).  The scheduler is host code; it adds nothing on the device."""
    cfg = pool.cfg
    n_req = len(requests)
    max_seqs = max(1, min(int(max_seqs), WIDE_MAX))
    row_budget = max(1, min(int(row_budget), MIXED_ROWS_MAX))
    max_seqs = min(max_seqs, row_budget)
    chunk = row_budget if chunk is None else max(1, int(chunk))
    prompts = [np.ascontiguousarray(r[0], np.int32).reshape(-1) for r in requests]
    max_new = [int(r[1]) for r in requests]
    for i in range(n_req):
        if not 1 <= prompts[i].size <= cfg.seq_len or max_new[i] < 1:
            raise ValueError(f"request {i}: {prompts[i].size} tokens (1 .. seq_len), max_new {max_new[i]} (at least 1)")
    temp = None if temperature is None else np.broadcast_to(np.asarray(temperature, np.float32), (n_req,))
    topp = np.broadcast_to(np.asarray(1.0 if top_p is None else top_p, np.float32), (n_req,))
    pages_of = [(min(prompts[i].size + max_new[i], cfg.seq_len) + KV_PAGE - 1) // KV_PAGE for i in range(n_req)]
    pages_free = pool.info()["n_free"]   # less what the requests in flight have been promised
    if any(p > pages_free for p in pages_of):
        raise ValueError("a request needs more pages than the pool has free")
    idle, flight, waiting = [], [], list(range(n_req))   # runstates; requests in flight, in arrival order; the queue
    fed = [0] * n_req            # rows of the request already run = its next position
    out = [[] for _ in range(n_req)]
    state_of = {}
    trace = []
    try:
        while flight or waiting:
            rows = {i: 1 for i in flight if fed[i] >= prompts[i].size}   # the decoders' rows first
            left = row_budget - len(rows)
            for i in flight:
                if i not in rows and left > 0:
                    rows[i] = min(chunk, left, prompts[i].size - fed[i])
                    left -= rows[i]
            while waiting and left > 0 and len(flight) < max_seqs and pages_of[waiting[0]] <= pages_free:
                i = waiting.pop(0)
                pages_free -= pages_of[i]
                if not idle:
                    idle.append(RunState(cfg, pool=pool))
                state_of[i] = idle.pop()
                flight.append(i)
                rows[i] = min(chunk, left, prompts[i].size)
                left -= rows[i]
            call = [i for i in flight if i in rows]   # (never empty: a decoder has its row, and an empty flight admits)
            lists, p0 = [], []
            for i in call:
                if fed[i] >= prompts[i].size:
                    lists.append([out[i][-1]])
                else:
                    lists.append(prompts[i][fed[i]: fed[i] + rows[i]])
                p0.append(fed[i])
            tp = pp = cp = None
            if temp is not None:
                tp, pp = [temp[i] for i in call], [topp[i] for i in call]
                cp = [float(coins[i][len(out[i])]) if tp[k] > 0 else 0.0 for k, i in enumerate(call)]
            nxt = step_mixed([state_of[i] for i in call], lists, p0, w, tp, pp, cp)
            held = [state_of[i].pages() for i in call]
            trace.append({"ids": list(call), "n_tokens": [int(rows[i]) for i in call], "pos0": list(p0),
                          "pages": [[int(p) for p in h[h >= 0]] for h in held]})
            for k, i in enumerate(call):
                fed[i] += rows[i]
                if fed[i] < prompts[i].size:
                    continue   # still in its prompt: the id is ignored
                out[i].append(int(nxt[k]))
                if out[i][-1] == bos or len(out[i]) >= max_new[i] or fed[i] >= cfg.seq_len:
                    s = state_of.pop(i)
                    s.trim(0)
                    idle.append(s)
                    flight.remove(i)
                    pages_free += pages_of[i]
    finally:
        for s in list(state_of.values()) + idle:
            s.close()
    return [np.asarray(o, np.int32) for o in out], trace


def runstate_fork(dst: RunState, src: RunState, n_pos: int) -> None:
    """l2z_runstate_fork: dst takes src's KV rows 0 .. n_pos-1 and its logits; dst's next position is n_pos."""
    _chk(lib().l2z_runstate_fork(dst.h, src.h, n_pos))


HOST_LIB_PATH = os.path.join(_HERE, "host", "libllama2_host.so")
_host = None


def host_lib():
    """libllama2_host.so: the host logic above the C ABI (tokenizer, samplers, the prompt-lookup drafter); no HIP."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise FileNotFoundError(f"{HOST_LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
        H = C.CDLL(HOST_LIB_PATH)
        H.l2zh_lookup_draft.argtypes = [C.POINTER(C.c_int32), C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        H.l2zh_lookup_draft.restype = C.c_size_t
        H.l2zh_lookup_draft_tree.argtypes = [C.POINTER(C.c_int32), C.c_size_t, C.c_int, C.c_int, C.c_int,
                                             C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        H.l2zh_lookup_draft_tree.restype = C.c_size_t
        H.l2zh_prng_floats.argtypes = [C.c_uint64, C.POINTER(C.c_float), C.c_size_t]
        H.l2zh_prng_floats.restype = None
        _host = H
    return _host


def lookup_draft(history, k: int, max_ngram: int = 3) -> np.ndarray:
    """Prompt-lookup drafter (l2zh_lookup_draft): for g = max_ngram .. 1 the most recent earlier occurrence of the last g
    tokens of `history`; the up to k tokens that followed it, or none."""
    h = np.ascontiguousarray(history, np.int32)
    out = np.zeros(max(int(k), 1), np.int32)
    i32p = C.POINTER(C.c_int32)
    n = host_lib().l2zh_lookup_draft(h.ctypes.data_as(i32p), h.size, int(max_ngram), int(k), out.ctypes.data_as(i32p))
    return out[:n].copy()


def lookup_draft_tree(history, depth: int, budget: int, max_ngram: int = 3):
    """Tree form of the prompt-lookup drafter (l2zh_lookup_draft_tree): EVERY earlier occurrence of the last g tokens of
    `history` (g = max_ngram .. 1, most recent first) contributes the up to `depth` tokens that followed it; the
    continuations are merged into a trie until `budget` (at most 15) guesses exist.  Returns (tokens, parent) of the
    guesses: guess k is tree node k + 1 (node 0 = the root, the sequence's last token), parent[k] its parent's tree node
    in [0, k].  The first continuation is lookup_draft(history, depth): guesses 0, 1, ... form that chain."""
    h = np.ascontiguousarray(history, np.int32)
    budget = max(0, min(int(budget), BATCH_MAX - 1))
    tok, par = np.zeros(max(budget, 1), np.int32), np.zeros(max(budget, 1), np.int32)
    i32p = C.POINTER(C.c_int32)
    n = host_lib().l2zh_lookup_draft_tree(h.ctypes.data_as(i32p), h.size, int(max_ngram), int(depth), budget,
                                          tok.ctypes.data_as(i32p), par.ctypes.data_as(i32p))
    return tok[:n].copy(), par[:n].copy()


def _check_guesses(what: str, n: int) -> None:
    if not 0 <= n <= BATCH_MAX - 1:
        raise ValueError(f"{what} = {n} outside [0, {BATCH_MAX - 1}]")


def _speculate_one(s: RunState, prompt, n_steps: int, prefill, guess_round, draw=None):
    """The loop behind speculate_greedy, speculate_sample, speculate_q8 and speculate_tree, which state its contract: the
    prompt's echo, prefill(BOS + prompt) and the first id -- s.argmax(), or with draw = (temperature, top_p, coins as an f32
    vector) sample_batch([s], temperature, top_p, coins[0]) --, then rounds until a BOS or n_steps positions.
    guess_round(hist, pos, room, g) makes one verify call at position pos and returns (ids, offered, accepted): hist is BOS
    and everything emitted, room the positions left behind pos, g the generated tokens so far = the index of the next coin,
    ids the sequence's next tokens, emitted as far as the run goes.  ValueError if the coins are too short for n_steps."""
    seq_len = s.cfg.seq_len
    steps = seq_len if n_steps == 0 else max(1, min(int(n_steps), seq_len))
    prompt = [int(t) for t in prompt][:steps]
    if draw is not None and draw[2].size < steps - len(prompt):
        raise ValueError(f"{draw[2].size} coins for {steps - len(prompt)} generated positions")
    hist, out = [1], []
    stats = {"calls": 0, "offered": 0, "accepted": 0, "emitted": 0}

    def emit(t):
        out.append(int(t))
        hist.append(int(t))
        return int(t) != 1

    alive, pos, g = True, 0, 0
    while alive and pos < len(prompt):
        alive = emit(prompt[pos])
        pos += alive
    if alive and pos < steps:
        prefill(np.array(hist, np.int32))
        alive = emit(s.argmax() if draw is None else sample_batch([s], draw[0], draw[1], draw[2][0])[0])
        g += 1
        pos += alive
    while alive and pos < steps:
        ids, offered, accepted = guess_round(hist, pos, steps - pos - 1, g)
        stats["calls"] += 1
        stats["offered"] += offered
        stats["accepted"] += accepted
        for t in ids:
            if not (alive and pos < steps):
                break
            alive = emit(t)
            stats["emitted"] += 1
            g += 1
            pos += alive
    return np.array(out, np.int32), stats


def _chain_round(k: int, drafter, verify):
    """_speculate_one's round for a chain of up to k guesses: drafter(history, kk), asked only for kk > 0 guesses, then
    verify(tokens, pos, g) -> (next, accepted) on the last id and the guesses."""
    if drafter is None:
        drafter = lookup_draft

    def guess_round(hist, pos, room, g):
        kk = min(k, room)
        guesses = [int(t) for t in drafter(np.array(hist, np.int32), kk)][:kk] if kk > 0 else []
        nxt, a = verify([hist[-1]] + guesses, pos, g)
        return nxt[: a + 1], len(guesses), a
    return guess_round


def _draw_of(temperature, top_p, coins):
    """speculate_q8's and speculate_tree's draw arguments as _speculate_one takes them: None at temperature None"""
    if temperature is None:
        return None
    return temperature, 1.0 if top_p is None else top_p, np.ascontiguousarray(coins, np.float32).reshape(-1)


def _draw_window(draw, g: int, n: int) -> tuple:
    """what a verify call of n positions at generated index g takes behind the weights: nothing, or the draw with its coins"""
    return () if draw is None else (draw[0], draw[1], draw[2][g: g + n])


def speculate_greedy(s: RunState, w: Weights, prompt, n_steps: int, k: int, drafter=None):
    """The loop of `llama2 -t 0 --spec k`: greedy decoding of n_steps positions (0 = seq_len) from BOS + prompt, up to k
    guessed tokens verified per sweep of the weights (RunState.verify).  drafter(history, k) -> guesses (history: BOS, then
    everything emitted; at most k ids are used); default lookup_draft.  Returns (tokens, stats): tokens = the `next` of
    every position from 0 as l2z_greedy_run reports them (prompt positions echo the prompt; a BOS ends the run and is the
    last id), stats = {"calls", "offered", "accepted", "emitted"} (emitted: ids that came out of verify calls).  The ids do
    not depend on k or on the drafter (DRAFT INVARIANCE)."""
    _check_guesses("k", k)
    return _speculate_one(s, prompt, n_steps, lambda t: s.prefill(t, 0, w),
                          _chain_round(k, drafter, lambda t, pos, g: s.verify(t, pos, w)))


def coin_stream(seed: int, n: int) -> np.ndarray:
    """The first n next_f32() of the CLI's Prng(seed) (l2zh_prng_floats): the coins of `llama2 -s seed`, one per
    generated token in generation order."""
    out = np.zeros(max(int(n), 1), np.float32)
    host_lib().l2zh_prng_floats(C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _fp(out), int(n))
    return out[: int(n)].copy()


def generate_sample(s: RunState, w: Weights, prompt, n_steps: int, temperature: float, top_p: float, coins) -> np.ndarray:
    """The loop of `llama2 -t temperature -p top_p` on the device: n_steps positions (0 = seq_len) from BOS + prompt in one
    RunState.sample_run call.  coins[g] is the coin of the g-th generated token (speculate_sample's convention, coin_stream's
    order); prompt steps get a coin of 0, which is not read.  Returns the `next` of every position from 0 as l2z_greedy_run
    reports them; a BOS ends the run and is the last id.  ValueError if `coins` is too short for n_steps."""
    seq_len = s.cfg.seq_len
    steps = seq_len if n_steps == 0 else max(1, min(int(n_steps), seq_len))
    prompt = [int(t) for t in prompt]
    n_gen = max(0, steps - len(prompt))
    per_step = np.zeros(steps, np.float32)
    if temperature > 0 and n_gen > 0:
        coins = np.ascontiguousarray(coins, np.float32).reshape(-1)
        if coins.size < n_gen:
            raise ValueError(f"{coins.size} coins for {n_gen} generated positions")
        per_step[len(prompt):] = coins[:n_gen]
    s.greedy_begin(prompt)
    return s.sample_run(w, steps, temperature, top_p, per_step)


def speculate_sample(s: RunState, w: Weights, prompt, n_steps: int, k: int, temperature: float, top_p: float, coins,
                     drafter=None):
    """The loop of `llama2 --spec-sample k`: speculate_greedy's loop and return convention with every generated token
    DRAWN (RunState.verify_sample).  coins[g] is the coin of the g-th generated token whatever call draws it: the first
    comes from the prefill's logits by sample_batch([s], ...) with coins[0]; a call at generated index g passes
    coins[g : g + 1 + len(guesses)]; a position behind a rejected guess is drawn again by the next call with the same
    coin.  The drafter must not look at the coins.  The ids do not depend on k or on the drafter (COIN INVARIANCE).
    ValueError if `coins` is too short for n_steps."""
    _check_guesses("k", k)
    draw = (temperature, top_p, np.ascontiguousarray(coins, np.float32).reshape(-1))
    return _speculate_one(s, prompt, n_steps, lambda t: s.prefill(t, 0, w),
                          _chain_round(k, drafter, lambda t, pos, g: s.verify_sample(t, pos, w, *_draw_window(draw, g, len(t)))),
                          draw)


def speculate_q8(s: RunState, w: Weights, prompt, n_steps: int, k: int, drafter=None, temperature=None, top_p=None, coins=None):
    """speculate_greedy's loop (temperature=None) or speculate_sample's on int8 group-quantized weights: RunState.prefill_q8
    for BOS + prompt, then up to k guessed tokens verified per sweep of the weights by RunState.verify_q8.  Arguments, the
    coins' convention (coins[g]: the coin of the g-th generated token) and the return value are theirs; the ids do not
    depend on k or on the drafter."""
    _check_guesses("k", k)
    draw = _draw_of(temperature, top_p, coins)
    return _speculate_one(s, prompt, n_steps, lambda t: s.prefill_q8(t, 0, w),
                          _chain_round(k, drafter, lambda t, pos, g: s.verify_q8(t, pos, w, *_draw_window(draw, g, len(t)))),
                          draw)


def speculate_tree(s: RunState, w: Weights, prompt, n_steps: int, depth: int, budget: int, drafter=None, temperature=None,
                   top_p=None, coins=None):
    """speculate_greedy's loop (temperature=None) or speculate_sample's with a TREE of guesses verified per sweep of the
    weights (RunState.verify_tree): up to `budget` guessed nodes, at most `depth` edges below the sequence's last token.
    drafter(history, depth, budget) -> (tokens, parent) of the guesses in lookup_draft_tree's convention, which is the
    default; nodes deeper than asked, beyond the budget or behind a dropped node are not used.  Sampled mode: coins[g] is
    the coin of the g-th generated token as in speculate_sample, so a call at generated index g passes
    coins[g : g + 1 + max depth].  The return convention is speculate_greedy's; stats["offered"] counts guessed nodes,
    stats["accepted"] edges walked.  The ids do not depend on depth, budget or the drafter (PATH INVARIANCE): they are
    speculate_greedy's, or speculate_sample's for the same coins."""
    _check_guesses("budget", budget)
    if drafter is None:
        drafter = lookup_draft_tree
    draw = _draw_of(temperature, top_p, coins)

    def guess_round(hist, pos, room, g):
        dd, bb = min(int(depth), room), min(int(budget), s.cfg.seq_len - pos - 1)
        tokens, parent, dep = [hist[-1]], [-1], [0]
        if dd > 0 and bb > 0:
            gt, gp = drafter(np.array(hist, np.int32), dd, bb)
            node = {0: 0}  # the drafter's tree node -> ours
            for k, (t, p) in enumerate(zip(gt, gp)):
                p = node.get(int(p))
                if p is None or dep[p] + 1 > dd or len(tokens) > bb:
                    continue
                node[k + 1] = len(tokens)
                tokens.append(int(t)); parent.append(p); dep.append(dep[p] + 1)
        nxt, path, a = s.verify_tree(tokens, parent, pos, w, *_draw_window(draw, g, 1 + max(dep)))
        return nxt[path], len(tokens) - 1, a

    return _speculate_one(s, prompt, n_steps, lambda t: s.prefill(t, 0, w), guess_round, draw)


def speculate_batch(states, w: Weights, prompts, n_steps: int, k: int, drafter=None, *, temperature=None, top_p=None,
                    coins=None, batched_prefill=True):
    """speculate_greedy's loop (temperature=None) or speculate_sample's for len(states) sequences at once: every round ONE
    verify_batch call advances all the sequences still running, each with min(k + 1, 16 // live) rows -- its last token and
    the drafter's guesses.  A sequence that emits BOS or reaches n_steps drops out.  Sampled mode: temperature and top_p are
    one value per sequence or a scalar, coins[j] is sequence j's coin stream indexed by generated token as in
    speculate_sample.  The prompts go through prefill_batch (batched_prefill=True: values agree with RunState.prefill's up
    to summation order) or through RunState.prefill per sequence (False: every sequence's ids are then speculate_greedy's /
    speculate_sample's on a fresh runstate, bit for bit, whatever the other sequences are).
    Returns (list of token arrays, stats): per sequence the return convention of speculate_greedy; stats is per call:
    speculate_greedy's keys plus "rows" (rows of all verify_batch calls) and "rows_per_call" (a list)."""
    return _speculate_rows(verify_batch, BATCH_MAX, False, states, w, prompts, n_steps, k, drafter, temperature, top_p, coins,
                           batched_prefill)


def speculate_wide(states, w: Weights, prompts, n_steps: int, k: int, drafter=None, *, temperature=None, top_p=None,
                   coins=None):
    """speculate_batch's loop over verify_wide, for up to WIDE_MAX sequences: every round ONE verify_wide call advances all
    the sequences still running.  Each asks for min(k + 1, 16) rows -- its last token and the drafter's guesses; when the
    rows asked for exceed WIDE_MAX the guesses are trimmed evenly (every sequence gets WIDE_MAX // live rows, the first
    WIDE_MAX % live one more).  The drafter, the position-indexed coins, the cut at BOS and the return convention are
    speculate_batch's; the prompts go through prefill_batch in groups of BATCH_MAX sequences.  The ids agree with
    speculate_batch's up to the fp32 parity bar: a verify_wide row's bits depend on the call's layout."""
    return _speculate_rows(verify_wide, WIDE_MAX, True, states, w, prompts, n_steps, k, drafter, temperature, top_p, coins, True)


def _speculate_rows(verify, n_max, spread, states, w, prompts, n_steps, k, drafter, temperature, top_p, coins, batched_prefill):
    """the loop speculate_batch and speculate_wide share; verify: verify_batch or verify_wide, for up to n_max sequences
    and as many rows a call; spread: the rows that n_max leaves over an even share go to the first sequences"""
    if not 0 <= k <= BATCH_MAX - 1:
        raise ValueError(f"k = {k} outside [0, {BATCH_MAX - 1}]")
    n = len(states)
    if not 1 <= n <= n_max or len(prompts) != n:
        raise ValueError(f"{n} runstates and {len(prompts)} prompts (1 .. {n_max}, one prompt each)")
    if drafter is None:
        drafter = lookup_draft
    sampled = temperature is not None
    seq_len = states[0].cfg.seq_len
    steps = seq_len if n_steps == 0 else max(1, min(int(n_steps), seq_len))
    prompts = [[int(t) for t in p][:steps] for p in prompts]
    if sampled:
        temps = np.broadcast_to(np.asarray(temperature, np.float32), (n,))
        tops = np.broadcast_to(np.asarray(1.0 if top_p is None else top_p, np.float32), (n,))
        if coins is None or len(coins) != n:
            raise ValueError("sampled mode takes one coin stream per sequence")
        coins = [np.ascontiguousarray(c, np.float32).reshape(-1) for c in coins]
        for j in range(n):
            if coins[j].size < steps - len(prompts[j]):
                raise ValueError(f"sequence {j}: {coins[j].size} coins for {steps - len(prompts[j])} generated positions")
    hist, out = [[1] for _ in range(n)], [[] for _ in range(n)]
    alive, pos, gen = [True] * n, [0] * n, [0] * n  # gen: generated tokens so far = the index of the next coin
    stats = {"calls": 0, "offered": 0, "accepted": 0, "emitted": 0, "rows": 0, "rows_per_call": []}

    def emit(j, t):
        out[j].append(int(t))
        hist[j].append(int(t))
        alive[j] = int(t) != 1
        pos[j] += alive[j]

    for j in range(n):
        while alive[j] and pos[j] < len(prompts[j]):
            emit(j, prompts[j][pos[j]])
    first = [j for j in range(n) if alive[j] and pos[j] < steps]
    if first:
        if batched_prefill:
            for g in range(0, len(first), BATCH_MAX):
                grp = first[g: g + BATCH_MAX]
                prefill_batch([states[j] for j in grp], [np.array(hist[j], np.int32) for j in grp], 0, w)
        else:
            for j in first:
                states[j].prefill(np.array(hist[j], np.int32), 0, w)
        ids = []
        for g in range(0, len(first), BATCH_MAX):
            grp = first[g: g + BATCH_MAX]
            if sampled:
                ids.extend(sample_batch([states[j] for j in grp], temps[grp], tops[grp], [coins[j][0] for j in grp]))
            else:
                ids.extend(argmax_batch([states[j] for j in grp]))
        for j, t in zip(first, ids):
            emit(j, t)
            gen[j] += 1
    while True:
        live = [j for j in range(n) if alive[j] and pos[j] < steps]
        if not live:
            break
        lists, clists = [], []
        share, over = divmod(n_max, len(live))
        for i, j in enumerate(live):
            rows_each = min(k + 1, BATCH_MAX, share + (spread and i < over))
            kk = min(rows_each - 1, steps - pos[j] - 1)
            guesses = [int(g) for g in drafter(np.array(hist[j], np.int32), kk)][:kk] if kk > 0 else []
            lists.append([hist[j][-1]] + guesses)
            if sampled:
                clists.append(coins[j][gen[j]: gen[j] + 1 + len(guesses)])
            stats["offered"] += len(guesses)
        if sampled:
            nxts, accs = verify([states[j] for j in live], lists, [pos[j] for j in live], w, temps[live], tops[live], clists)
        else:
            nxts, accs = verify([states[j] for j in live], lists, [pos[j] for j in live], w)
        stats["calls"] += 1
        stats["rows"] += sum(len(t) for t in lists)
        stats["rows_per_call"].append(sum(len(t) for t in lists))
        for j, nxt, a in zip(live, nxts, accs):
            stats["accepted"] += int(a)
            for t in nxt[: int(a) + 1]:
                if not (alive[j] and pos[j] < steps):
                    break
                emit(j, t)
                stats["emitted"] += 1
                gen[j] += 1
    return [np.array(o, np.int32) for o in out], stats


def emu_transformer(states, weights, token: int, pos: int) -> None:
    """One forward pass of N emulated ranks on one GPU (l2z_emu_transformer)."""
    n = len(states)
    ss = (C.c_void_p * n)(*[s.h for s in states])
    ws = (C.c_void_p * n)(*[w.h for w in weights])
    _chk(lib().l2z_emu_transformer(n, ss, ws, token, pos))


def prefill_attention(form: int, q, kcache, vcache, pos0: int, n_heads: int, n_kv_heads: int, head_size: int) -> np.ndarray:
    """The batched prefill's attention kernels on (q [P, dim], caches [seq_len, kv_dim]); form as in the header."""
    q, kcache, vcache = _f32(q), _f32(kcache), _f32(vcache)
    out = np.empty_like(q)
    _chk(lib().l2z_prefill_attention(form, _fp(out), _fp(q), _fp(kcache), _fp(vcache), pos0, q.shape[0], n_heads,
                                     n_kv_heads, head_size, kcache.shape[0]))
    return out


def shard_plan(cfg, rank: int, world: int) -> dict:
    """What rank `rank` of `world` owns (host logic, no device): scheme A's row / head ranges and scheme B's padded widths."""
    buf = (C.c_int * 10)()
    c = _cfg(cfg)
    _chk(lib().l2z_shard_plan(C.byref(c), rank, world, buf, 10))
    keys = ("dim0", "dim_loc", "kvd_loc", "heads_loc", "hid0", "hid_loc", "v0", "v_loc", "dimc_pad", "hidc_pad")
    return dict(zip(keys, list(buf)))


def prefill_plan(n_tokens: int, cfg=None) -> list[int]:
    """Chunk lengths of a batched prefill of n_tokens (host logic, no device); with a config: of that model's."""
    buf = (C.c_int * 64)()
    if cfg is not None:
        c = _cfg(cfg)
        n = lib().l2z_prefill_plan_model(C.byref(c), n_tokens, buf, 64)
    else:
        n = lib().l2z_prefill_plan(n_tokens, buf, 64)
    if n < 0:
        raise L2ZError(n, lib().l2z_last_error().decode(errors="replace"))
    return list(buf[:n])


TILE_FORMS = ("128x64", "64x64", "32x64", "32x32", "128x128")


def prefill_tile(n_features: int, n_tokens: int, paired: bool = False) -> str:
    """Output tile the direct-to-LDS GEMM takes for an [n_tokens, n_features] product (host logic)."""
    t = lib().l2z_prefill_tile(n_features, n_tokens, 1 if paired else 0)
    if t < 0:
        raise L2ZError(t, lib().l2z_last_error().decode(errors="replace"))
    return TILE_FORMS[t]


def prefill_split_k(n_features_whole: int, n_tokens: int, k: int, paired: bool = False) -> int:
    """K ranges per output tile the tile GEMM takes for this product (host logic; 1 = the unsplit family)."""
    r = lib().l2z_prefill_split_k(n_features_whole, n_tokens, k, 1 if paired else 0)
    if r < 0:
        raise L2ZError(r, lib().l2z_last_error().decode(errors="replace"))
    return r


class GemmShape(C.Structure):
    """include/llama2_hip_test.h l2z_gemm_shape."""
    _fields_ = [(n, C.c_int) for n in ("kind", "epi", "n_tokens", "n_features", "k", "ldx", "n_scale", "sk", "nq", "nkv",
                                       "w13_one_matrix", "cnt_ints")] + [("n_launch_whole", C.c_longlong), ("part_floats", C.c_longlong)]


class GemmPlan(C.Structure):
    """include/llama2_hip_test.h l2z_gemm_plan."""
    _fields_ = [(n, C.c_int) for n in ("family", "epi", "k", "x3", "sk", "tile", "feat", "tm", "nbuf", "one_round", "tms", "paired")]


GEMM_KINDS = ("single", "qkv", "w13", "kv")
GEMM_FAMILIES = {-1: "invalid", -2: "not supported", -3: "no workspace", 1: "stream", 2: "short", 3: "split-k", 4: "two-block", 5: "tile"}


def prefill_gemm_plan(kind: str, n_tokens: int, n_features: int, k: int, **kw) -> dict:
    """The kernel form a product of the batched prefill takes (host logic): l2z_prefill_gemm_plan's plan as a dict, `family`
    and `tile` by name.  kw: the other fields of l2z_gemm_shape; ldx defaults to the pass's padded rows (multiples of 256,
    at least 768), the workspace to a large one."""
    sh = GemmShape(kind=GEMM_KINDS.index(kind), n_tokens=n_tokens, n_features=n_features, k=k, n_scale=1, sk=1,
                   ldx=max(768, (k + 255) // 256 * 256), part_floats=1 << 40, cnt_ints=1 << 16)
    for name, v in kw.items():
        if name not in dict(GemmShape._fields_):
            raise TypeError(name)
        setattr(sh, name, int(v))
    pl = GemmPlan()
    _chk(lib().l2z_prefill_gemm_plan(C.byref(sh), C.byref(pl)))
    d = {n: getattr(pl, n) for n, _ in GemmPlan._fields_}
    d["family"], d["tile"] = GEMM_FAMILIES[pl.family], TILE_FORMS[pl.tile]
    return d


def prefill_cores(n_features_whole: int, n_tokens: int, k: int) -> int:
    """Matrix cores of a prefill product (host logic): 0 f32, 1 bf16 over three-term splits (tile forms), n >= 2 the
    stream form of the bf16 kernel with n - 1 K ranges."""
    r = lib().l2z_prefill_cores(n_features_whole, n_tokens, k)
    if r < 0:
        raise L2ZError(r, lib().l2z_last_error().decode(errors="replace"))
    return r


def prefill_on_bf16_cores(cfg) -> bool:
    """Whether the model's widest product (W1 | W3) multiplies on the bf16 matrix cores in the batched prefill."""
    return prefill_cores(2 * cfg.hidden_dim, 512, cfg.dim) > 0


def emu_prefill(states, weights, tokens, pos0: int) -> None:
    """l2z_prefill for N emulated ranks on one GPU (l2z_emu_prefill)."""
    n = len(states)
    ss = (C.c_void_p * n)(*[s.h for s in states])
    ws = (C.c_void_p * n)(*[w.h for w in weights])
    t = np.ascontiguousarray(tokens, dtype=np.int32)
    _chk(lib().l2z_emu_prefill(n, ss, ws, t.ctypes.data_as(C.POINTER(C.c_int32)), len(t), pos0))


# ---- kernel-level hooks (names follow src/main.zig) ----
def matmul(x, w) -> np.ndarray:
    x, w = _f32(x), _f32(w)
    d, n = w.shape
    out = np.empty(d, np.float32)
    _chk(lib().l2z_matmul(_fp(out), _fp(x), _fp(w), n, d))
    return out


def matmul_fused(x, ws) -> list[np.ndarray]:
    x = _f32(x)
    ws = [_f32(w) for w in ws]
    d, n = ws[0].shape
    outs = [np.empty(d, np.float32) for _ in ws]
    FP = C.POINTER(C.c_float)
    N = len(ws)
    _chk(lib().l2z_matmul_fused(N, (FP * N)(*[_fp(o) for o in outs]), _fp(x),
                                (FP * N)(*[_fp(w) for w in ws]), n, d))
    return outs


def rmsnorm(x, w) -> np.ndarray:
    x, w = _f32(x), _f32(w)
    o = np.empty_like(x)
    _chk(lib().l2z_rmsnorm(_fp(o), _fp(x), _fp(w), x.size))
    return o


def softmax(x) -> np.ndarray:
    o = np.array(x, np.float32, copy=True)
    _chk(lib().l2z_softmax(_fp(o), o.size))
    return o


def vector_dot_product(x, y) -> np.float32:
    x, y = _f32(x), _f32(y)
    o = np.zeros(1, np.float32)
    _chk(lib().l2z_vector_dot_product(_fp(o), _fp(x), _fp(y), x.size))
    return o[0]


def vector_weighted_sum_rows(xout_len: int, rows, row_stride: int, weights) -> np.ndarray:
    rows, weights = _f32(rows), _f32(weights)
    o = np.empty(xout_len, np.float32)
    _chk(lib().l2z_vector_weighted_sum_rows(_fp(o), xout_len, _fp(rows), rows.size, row_stride,
                                            _fp(weights), weights.size))
    return o


ATTN_FORMS = {"auto": 0, "fast256": 1, "fast1024": 2, "split": 3, "generic": 4}


def attention_decode(q, kcache, vcache, pos: int, n_heads: int, n_kv_heads: int, head_size: int,
                     seq_len: int, form: str = "auto", nch: int = 0) -> np.ndarray:
    """One layer's decode attention (src/main.zig:361-389) through the forward pass's kernels."""
    q, kcache, vcache = _f32(q), _f32(kcache), _f32(vcache)
    assert q.size == n_heads * head_size and kcache.size == seq_len * n_kv_heads * head_size
    out = np.empty(n_heads * head_size, np.float32)
    _chk(lib().l2z_attention_decode(ATTN_FORMS[form], nch, _fp(out), _fp(q), _fp(kcache), _fp(vcache),
                                    pos, n_heads, n_kv_heads, head_size, seq_len))
    return out


def q8_quantize(x, gs: int):
    """The activation rule of the int8 group quantization on the device: (q int8 [n], s f32 [n // gs])."""
    x = _f32(x).reshape(-1)
    q = np.empty(x.size, np.int8)
    s = np.empty(x.size // gs, np.float32)
    _chk(lib().l2z_q8_quantize(_fp(x), x.size, gs, q.ctypes.data_as(C.POINTER(C.c_int8)), _fp(s)))
    return q, s


def q8_matmul(xq, xs, wq, ws, gs: int) -> np.ndarray:
    """The quantized product on its own, through the pass's kernel body: wq [d, n] int8, ws [d, n // gs], xq [n], xs [n // gs]."""
    wq = np.ascontiguousarray(wq, dtype=np.int8)
    d, n = wq.shape
    xq = np.ascontiguousarray(xq, dtype=np.int8).reshape(-1)
    xs, ws = _f32(xs).reshape(-1), _f32(ws).reshape(-1)
    assert xq.size == n and xs.size == n // gs and ws.size == d * (n // gs)
    out = np.empty(d, np.float32)
    i8p = C.POINTER(C.c_int8)
    _chk(lib().l2z_q8_matmul(_fp(out), xq.ctypes.data_as(i8p), _fp(xs), wq.ctypes.data_as(i8p), _fp(ws), n, d, gs))
    return out


def q8_quantize_rows(x, gs: int, rms_w=None):
    """The row launch of the quantized prompt pass on its own (l2z_q8_quantize_rows): x [m, n] -> (q int8 [m, n], s f32
    [m, n // gs]) by the activation rule, after the rmsnorm with rms_w [n] where given."""
    x = _f32(x)
    assert x.ndim == 2
    m, n = x.shape
    g = None if rms_w is None else _f32(rms_w).reshape(-1)
    assert g is None or g.size == n
    q = np.empty((m, n), np.int8)
    s = np.empty((m, n // gs), np.float32)
    _chk(lib().l2z_q8_quantize_rows(_fp(x), m, n, None if g is None else _fp(g), gs, q.ctypes.data_as(C.POINTER(C.c_int8)), _fp(s)))
    return q, s


def q8_gemm(xq, xs, wq, ws, gs: int) -> np.ndarray:
    """The GEMM of the quantized prompt pass on its own, store epilogue (l2z_q8_gemm): xq [m, n] int8, xs [m, n // gs], wq
    [d, n] int8, ws [d, n // gs] -> out [m, d]."""
    xq = np.ascontiguousarray(xq, dtype=np.int8)
    wq = np.ascontiguousarray(wq, dtype=np.int8)
    (m, n), d = xq.shape, wq.shape[0]
    xs, ws = _f32(xs).reshape(-1), _f32(ws).reshape(-1)
    assert wq.shape[1] == n and xs.size == m * (n // gs) and ws.size == d * (n // gs)
    out = np.empty((m, d), np.float32)
    i8p = C.POINTER(C.c_int8)
    _chk(lib().l2z_q8_gemm(_fp(out), xq.ctypes.data_as(i8p), _fp(xs), m, wq.ctypes.data_as(i8p), _fp(ws), n, d, gs))
    return out


def generate_q8(s: RunState, w: Weights, prompt, n_steps: int, bos: int = 1) -> np.ndarray:
    """The greedy loop on int8 group-quantized weights with a batched prompt pass: prefill_q8 of BOS + prompt at position 0,
    then transformer + argmax per step.  Returns the `next` of every position from 0 as l2z_greedy_run reports them (the
    prompt's tokens, then the picks); a BOS ends the run and is the last id."""
    prompt = [int(t) for t in prompt]
    steps = s.cfg.seq_len if n_steps == 0 else max(1, min(int(n_steps), s.cfg.seq_len))
    fed = ([bos] + prompt)[:steps]
    s.prefill_q8(fed, 0, w)
    ids = prompt[:len(fed) - 1]
    tok = s.argmax() if len(fed) > len(prompt) else prompt[len(fed) - 1]
    ids.append(tok)
    for pos in range(len(fed), steps):
        if tok == bos:
            break
        s.transformer(tok, pos, w)
        tok = s.argmax()
        ids.append(tok)
    return np.array(ids, np.int32)


def _q8_case_fields():
    i8p, fp = C.POINTER(C.c_int8), C.POINTER(C.c_float)
    return ([(n, C.c_int) for n in ("epi", "gs", "n", "rows0", "rows1", "rows2")] +
            [(n, i8p) for n in ("q0", "q1", "q2")] + [(n, fp) for n in ("s0", "s1", "s2")] +
            [("xq", i8p), ("xs", fp), ("x", fp), ("rms_w", fp)] +
            [(n, C.c_int) for n in ("pos", "head_size", "rope_segs", "seq_len")] +
            [("rope", fp), ("resid", fp), ("in_place", C.c_int), ("max_blocks_per_cu", C.c_int), ("n_cus", C.c_int)] +
            [(n, fp) for n in ("out0", "out1", "out2")] + [(n, C.c_size_t) for n in ("out0_len", "out1_len", "out2_len")] +
            [("part_val", fp), ("part_idx", C.POINTER(C.c_int)), ("part_cap", C.c_int), ("grid", C.c_int)])


class Q8Case(C.Structure):
    """include/llama2_hip_test.h l2z_q8_case."""
    _fields_ = _q8_case_fields()


Q8_EPIS = ("store", "rope", "resid", "swiglu", "argmax")


def q8_matvec_case(epi: str, gs: int, segs, *, xq=None, xs=None, x=None, rms_w=None, outs=None, rope=None, pos: int = 0,
                   head_size: int = 0, rope_segs: int = 0, seq_len: int = 0, resid=None, in_place: bool = False,
                   max_blocks_per_cu: int = 0, n_cus: int = 0) -> dict:
    """One launch of the quantized mat-vec as the pass issues it (l2z_q8_matvec_case).  segs: up to three (wq [rows, n] int8,
    ws [rows, n // gs]); "swiglu": ONE entry, the 2 * pairs rows of W1 | W3 interleaved.  x: (xq, xs), or f32 x, or f32 x
    with rms_w (the rmsnorm in the kernel).  outs: the output buffers as they stand before the launch (default: zeros of
    the segments' rows; "rope": q, then the head-major K and V caches [kv heads, seq_len, head_size]); "resid" with in_place:
    outs[0] is the residual.  rope: [pos + 1, head_size // 2, 2] cos / sin.  Returns {"outs", "grid", "n_pairs"} and, for
    "argmax", "part_val" / "part_idx" (one candidate a block)."""
    c = Q8Case()
    keep = []   # (the arrays the structure points into)

    def ptr(a, dtype, ctype):
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ctype))

    c.epi, c.gs = Q8_EPIS.index(epi), gs
    mats = [(np.ascontiguousarray(q, dtype=np.int8), _f32(s)) for q, s in segs]
    n = mats[0][0].shape[1]
    assert 1 <= len(mats) <= 3 and all(q.ndim == 2 and q.shape[1] == n and s.size == q.shape[0] * (n // gs) for q, s in mats)
    rows = [q.shape[0] for q, _ in mats]
    if epi == "swiglu":
        assert len(mats) == 1 and rows[0] % 2 == 0
        rows = [rows[0] // 2, rows[0] // 2]
    c.n = n
    c.rows0, c.rows1, c.rows2 = (rows + [0, 0])[:3]
    for j, (q, s) in enumerate(mats):
        setattr(c, f"q{j}", ptr(q, np.int8, C.c_int8))
        setattr(c, f"s{j}", ptr(s, np.float32, C.c_float))
    if xq is not None:
        assert np.size(xq) == n and np.size(xs) == n // gs and x is None and rms_w is None
        c.xq, c.xs = ptr(xq, np.int8, C.c_int8), ptr(xs, np.float32, C.c_float)
    else:
        assert np.size(x) == n and (rms_w is None or np.size(rms_w) == n)
        c.x = ptr(x, np.float32, C.c_float)
        if rms_w is not None:
            c.rms_w = ptr(rms_w, np.float32, C.c_float)
    n_out = 1 if epi == "swiglu" else len(mats)
    if outs is None:
        assert epi != "rope", "rope: pass q and the two caches"
        outs = [np.zeros(r, np.float32) for r in rows[:n_out]]
    assert len(outs) == n_out
    outs = [np.array(o, dtype=np.float32, order="C") for o in outs]   # copies: the launch writes into them
    for j, o in enumerate(outs):
        setattr(c, f"out{j}", o.ctypes.data_as(C.POINTER(C.c_float)))
        setattr(c, f"out{j}_len", o.size)
    if epi == "rope":
        rope = _f32(rope)
        assert rope.size == (pos + 1) * (head_size // 2) * 2
        c.rope = ptr(rope, np.float32, C.c_float)
        c.pos, c.head_size, c.rope_segs, c.seq_len = pos, head_size, rope_segs, seq_len
    if epi == "resid":
        c.in_place = int(in_place)
        if not in_place:
            assert np.size(resid) == rows[0]
            c.resid = ptr(resid, np.float32, C.c_float)
    c.max_blocks_per_cu, c.n_cus = max_blocks_per_cu, n_cus
    part_val, part_idx = np.zeros(8192, np.float32), np.zeros(8192, np.int32)
    if epi == "argmax":
        c.part_val, c.part_idx, c.part_cap = _fp(part_val), part_idx.ctypes.data_as(C.POINTER(C.c_int)), part_val.size
    _chk(lib().l2z_q8_matvec_case(C.byref(c)))
    res = {"outs": outs, "grid": int(c.grid), "n_pairs": rows[0] if epi == "swiglu" else (sum(rows) + 1) // 2}
    if epi == "argmax":
        res["part_val"], res["part_idx"] = part_val[: c.grid].copy(), part_idx[: c.grid].copy()
    return res


def rccl_info() -> dict:
    """Loads RCCL now; {'path': the file the process got, 'version': ncclGetVersion's code}."""
    buf, v = C.create_string_buffer(512), C.c_int(0)
    _chk(lib().l2z_comm_rccl_info(buf, 512, C.byref(v)))
    return {"path": buf.value.decode(errors="replace"), "version": v.value}


def option_set(name: str, value: int) -> None:
    """A tuning knob of csrc/tunables.h by its environment name; applies to objects created afterwards."""
    _chk(lib().l2z_option_set(name.encode(), int(value)))


def argmax(x) -> int:
    x = _f32(x)
    i = C.c_size_t(0)
    _chk(lib().l2z_argmax_host(_fp(x), x.size, C.byref(i)))
    return int(i.value)
