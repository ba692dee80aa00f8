"""The case table of scripts/prefill_hash.py -- the bit-equality check of the prefill GEMM kernels between two builds --
against the plan hook (host logic, no device: 256 CUs assumed): every case's products take the kernel form the case is
there for, and the table as a whole reaches every form of prefill_gemm.hip's two kernels, the short-prompt kernels and the
panel kernel."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ph(B):
    spec = importlib.util.spec_from_file_location("prefill_hash", os.path.join(ROOT, "scripts", "prefill_hash.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.B is B   # (the one package: the options set below are the ones the plans read)
    for k, v in mod.DEFAULTS.items():
        B.option_set(k, v)
    return mod


def test_every_case_takes_the_form_it_is_there_for(ph):
    assert len({c[0] for c in ph.CASES}) == len(ph.CASES)
    for case in ph.CASES:
        ph.check_case(case)
    # a chunk that may go to the panel kernel instead of the planned forms says which: either the case is a panel case, or the
    # panel kernel is switched off, or the chunk is one the kernel never takes (above 96 tokens; below 17; 33 tokens and up on
    # the bf16 cores, where the stream form takes every matrix that streams; a cache-resident model)
    # (The limits written out below are the kernels' own: csrc/prefill_panel.hip prefill_panel_shape -- kPanelDefaultMin = 17 up
    # to prefill_panel_max_tokens() = 96 tokens, matrices of more than 16 MB over the whole model, for which dim >= 2048 stands
    # here -- and csrc/prefill_gemm.hip x3_stream_shape, which takes such matrices from L2Z_PF_X3_STREAM_MIN = 33 tokens on the
    # bf16 cores.  If those move, this rule moves with them.)
    for name, model, P, opts, want in ph.CASES:
        x3 = opts.get("L2Z_PF_X3", ph.DEFAULTS["L2Z_PF_X3"])
        in_range = 17 <= P <= (96 if x3 == 0 else 32) and ph.MODELS[model]["dim"] >= 2048
        assert want == "panel" or not in_range or opts.get("L2Z_PF_PANEL") == 0, name


def test_the_table_reaches_every_form(ph, B):
    """(family, what distinguishes the form) of every product of every case, under the case's options."""
    seen, panel = [], []
    for name, model, P, opts, want in ph.CASES:
        for k, v in opts.items():
            B.option_set(k, v)
        try:
            if want == "panel":
                panel.append(P)
                continue
            got = ph.products(ph.MODELS[model], P)
            seen += [(prod, got[prod]) for prod in want]   # (only the products the case names and check_case pinned)
        finally:
            for k in opts:
                B.option_set(k, ph.DEFAULTS[k])

    def reached(family, **fields):
        return any(pl["family"] == family and all(pl[f] == v for f, v in fields.items()) for _, pl in seen)

    def reached_by(prods, family, **fields):
        return any(prod in prods and pl["family"] == family and all(pl[f] == v for f, v in fields.items()) for prod, pl in seen)

    for tile in ("128x64", "64x64", "32x64", "32x32", "128x128"):   # the tile kernel, every tile form, on the f32 cores
        assert reached("tile", tile=tile, x3=0), tile
    assert reached("tile", x3=1)
    for sk in (2, 4):   # split-K: the residual products, the pair, q | k | v fused
        assert reached_by(("wo", "w2"), "split-k", sk=sk, epi=1) and reached_by(("w13",), "split-k", sk=sk, epi=0) and \
            reached_by(("qkv",), "split-k", sk=sk, epi=6), sk
    assert reached_by(("wo", "w2"), "two-block", epi=1) and reached_by(("w13",), "two-block", epi=0) and reached_by(("qkv",), "two-block", epi=6)
    for feat in (128, 192, 256):
        assert reached("stream", feat=feat), feat
    for tm in (2, 4):
        assert reached("stream", tm=tm), tm
    for sk in (2, 4, 8):
        assert reached("stream", sk=sk), sk
    # the stream form's launches of several rounds (the last arriver of a tile adds the ranges): the W1 | W3 product of a
    # 19200-wide hidden layer at 100 tokens -- 300 tiles of 128 features x 2 ranges on 256 CUs -- is a one-layer shape
    assert reached("stream", one_round=0) and any(pl["family"] == "stream" and pl["one_round"] == 0 and pl["sk"] > 1 for _, pl in seen)
    assert reached("stream", one_round=1, sk=8)
    assert reached("short", tms=1, paired=0) and reached("short", tms=2, paired=0) and reached("short", tms=1, paired=1)
    assert panel and all(P in (32, 48) for P in panel)   # (check_case held each to the planner's witness, which answers there only)
    assert reached("tile", k=320) and "15m" in ph.MODELS and ph.MODELS["15m"]["dim"] == 288   # K = 288, walked as 320
