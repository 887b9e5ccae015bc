"""CPU-only sweep of the token GEMM's launch plan (gemm.hip gemm_plan through fg_op_gemm_plan): for every shape, flavour, epilogue,
gate period, scratch setting, tile order and CU count the plan must describe launches whose workgroups visit every (token tile, output
tile, k piece) exactly once, within the limits of the kernel it names.  Nothing is launched; no GPU is needed.  (The anchor rows and
the refusal model hold with FASTGEN_AMD_GEMM_PP / FASTGEN_AMD_GEMM_NARROW unset, as the plan reads them once per process.)"""
import ctypes
import functools
import itertools

import numpy as np
import pytest

from fastgen_amd import _lib
from fastgen_amd._lib import (FG_GEMM_EPI_HEADS, FG_GEMM_EPI_HEADS32, FG_GEMM_EPI_RAW, FG_GEMM_EPI_SPLIT, FG_GEMM_EPI_TOK, FG_GEMM_EPI_TOK32,
                              FG_GEMM_PP, FG_GEMM_PP_NARROW, FG_GEMM_PP_SPLITK, FG_GEMM_REFUSE_ARG, FG_GEMM_REFUSE_FORM, FG_GEMM_REFUSE_OFFSET,
                              FG_GEMM_REFUSE_PIECE, FG_GEMM_REG)

BF16, X3, FP8 = 0, 1, 2
GIB2 = 1 << 31
A_ROW = {BF16: lambda k: 2 * k, X3: lambda k: 4 * k, FP8: lambda k: k}        # bytes per row of A: bf16 / [hi | lo] planes / e4m3
O_ROW = {BF16: lambda n: 2 * n, X3: lambda n: 4 * n, FP8: lambda n: 2 * n}    # ... of out and resid: bf16 / fp32 or planes / bf16
W_ELEM = {BF16: 2, X3: 6, FP8: 1}                                             # bytes of W per (n, k): x3 packs [hi | lo | hi]
ORDER_BITS = {BF16: 127 | 256, X3: 15, FP8: 31}
FIELDS = ("refusal", "kernel", "tile_n", "epilogue", "ksplit", "xn", "grid", "lds_bytes", "row0", "rows", "pieces")

_plan = _lib.fg_gemm_plan()
_ref = ctypes.byref(_plan)


def plan(fl, m, n, k, heads=0, gate_rows=0, scratch=0, order=1, out_mode=0, cus=256, piece=0):
    """The plan's members as a tuple in FIELDS order."""
    assert _lib.lib().fg_op_gemm_plan(fl, m, n, k, heads, gate_rows, scratch, order, out_mode, cus, piece, _ref) == 0
    p = _plan
    return (p.refusal, p.kernel, p.tile_n, p.epilogue, p.ksplit, p.xn, p.grid, p.lds_bytes, p.row0, p.rows, p.pieces)


@functools.lru_cache(maxsize=None)
def walk_is_exact(rows, n, tile_n, ks, xn, grid):
    """Walks the work items of every workgroup with the kernels' own integer expressions (gemm_bf16_kernel / gemm_bf16_pp_kernel /
    gemm_bf16_pp2_kernel: mlo, nlo, nx, first, stride, count; with split-K an item is (tile, k piece) = (item / ks, item % ks)) and says
    whether every (token tile, output tile, k piece) was visited exactly once."""
    Mt, Nt = (rows + 255) // 256, (n + tile_n - 1) // tile_n
    hits = np.zeros(Mt * Nt * ks, dtype=np.int64)
    for block in range(grid):
        mlo, nlo, nx = 0, 0, Nt
        if (grid & 7) == 0 and xn > 0:
            x, xm = block & 7, 8 // xn
            xi = x // xn
            xj = x - xi * xn
            mlo, mhi = xi * Mt // xm, (xi + 1) * Mt // xm
            nlo = xj * Nt // xn
            nx = (xj + 1) * Nt // xn - nlo
            first, stride, count = block >> 3, grid >> 3, (mhi - mlo) * nx
        else:
            first, stride, count = block, grid, Mt * Nt
        count *= ks
        if first >= count:
            continue
        item = np.arange(first, count, stride, dtype=np.int64)
        lt = item // ks
        q = lt // nx
        mt, nt = mlo + q, nlo + (lt - q * nx)
        if mt.max() >= Mt or nt.max() >= Nt:
            return False
        np.add.at(hits, (mt * Nt + nt) * ks + item % ks, 1)
    return bool((hits == 1).all())


def refusal_model(fl, m, n, k, heads, gate_rows, order, out_mode):
    """The launchers' refusal rules written out a second time (gemm_bf16_supported / gemm_fp8_supported, launch_gemm_x3's checks, the
    2 GiB limits, fp32 out and the fp8 head split needing the ping-pong kernel, the x3 piece of at least one tile): 0 or the code."""
    if order & ~ORDER_BITS[fl] or bin(order & (16 | 32 | 256)).count("1") > 1 or out_mode not in ((0,) if fl == FP8 else (0, 1)):
        return FG_GEMM_REFUSE_ARG
    if n * k * W_ELEM[fl] >= GIB2:
        return FG_GEMM_REFUSE_OFFSET
    if k % (128 if fl == FP8 else 64) or n % 16 or (fl == X3 and (m < 256 or n < 256)):
        return FG_GEMM_REFUSE_ARG
    if heads:
        hd = n // (3 * heads)
        if n != 3 * heads * hd or hd % (8 if fl == X3 else 4) or (fl == FP8 and (heads * hd) % 8):
            return FG_GEMM_REFUSE_ARG
    rows_max = (GIB2 - 1) // max(A_ROW[fl](k), O_ROW[fl](n)) // 256 * 256
    if rows_max == 0:
        return FG_GEMM_REFUSE_OFFSET
    pieces = (m + rows_max - 1) // rows_max
    last = m - (pieces - 1) * rows_max
    if fl == X3:
        return FG_GEMM_REFUSE_PIECE if last < 256 else 0
    pp = lambda rows: not order & 16 and rows >= 256 and n >= 256 and k >= (256 if fl == FP8 else 128) and (not gate_rows or gate_rows >= 256)
    if fl == BF16 and out_mode == 1 and (heads or pieces > 1 or not pp(m)):
        return FG_GEMM_REFUSE_FORM
    if fl == FP8 and heads and not (pp(last) and pp(min(m, rows_max))):
        return FG_GEMM_REFUSE_FORM
    return 0


def violations(fl, m, n, k, heads, gate_rows, scratch, order, out_mode, cus):
    """The names of the invariants the plans of this call break (empty: none)."""
    p0 = plan(fl, m, n, k, heads, gate_rows, scratch, order, out_mode, cus, 0)
    want = refusal_model(fl, m, n, k, heads, gate_rows, order, out_mode)
    if p0[0] or want:
        if p0[0] != want:
            return ["refusal %d, the launchers' rules say %d" % (p0[0], want)]
        return [] if p0[1:] == (0,) * 10 else ["a refused plan with members set"]
    bad = []
    pieces = p0[10]
    if order & 64 and fl == BF16:
        scratch = max(scratch, 16 * m * n)
    row = 0
    for piece in range(pieces):
        p = p0 if piece == 0 else plan(fl, m, n, k, heads, gate_rows, scratch, order, out_mode, cus, piece)
        refusal, kernel, tile_n, epi, ks, xn, grid, lds, row0, rows, npieces = p
        if refusal or npieces != pieces:
            return ["piece %d refused or another piece count" % piece]
        # the pieces tile [0, m); all but the last are whole tiles; byte offsets into A, out and resid stay below 2 GiB
        if row0 != row or rows < 1 or (piece < pieces - 1 and rows % 256):
            bad.append("row pieces")
        row += rows
        if rows * A_ROW[fl](k) >= GIB2 or rows * O_ROW[fl](n) >= GIB2:
            bad.append("a piece past 2 GiB")
        # the kernel form, its tile and its epilogue belong together
        if (kernel, tile_n) not in ((FG_GEMM_REG, 256), (FG_GEMM_REG, 192), (FG_GEMM_PP, 256), (FG_GEMM_PP_NARROW, 128), (FG_GEMM_PP_SPLITK, 256)):
            bad.append("kernel form and tile width")
        if kernel == FG_GEMM_REG and (tile_n == 192) != (n % 256 != 0 and n % 192 == 0):
            bad.append("the 192-wide tile rule moved")
        if fl == X3:
            if kernel != FG_GEMM_PP or epi != (FG_GEMM_EPI_HEADS32 if heads else FG_GEMM_EPI_SPLIT if out_mode else FG_GEMM_EPI_TOK32):
                bad.append("split-bf16 form")
        elif kernel == FG_GEMM_PP_SPLITK:
            if epi != FG_GEMM_EPI_RAW:
                bad.append("split-K epilogue")
        elif epi != (FG_GEMM_EPI_HEADS if heads else FG_GEMM_EPI_TOK32 if out_mode else FG_GEMM_EPI_TOK):
            bad.append("epilogue")
        if (fl == FP8 or heads or out_mode or pieces > 1) and kernel not in (FG_GEMM_REG, FG_GEMM_PP):
            bad.append("narrow tile or split-K where only the token epilogue of one launch has them")
        if kernel == FG_GEMM_REG and (epi not in (FG_GEMM_EPI_TOK, FG_GEMM_EPI_HEADS) or (fl == FP8 and epi != FG_GEMM_EPI_TOK)):
            bad.append("an epilogue the register-staged kernel does not have")
        if order & 16 and kernel != FG_GEMM_REG:
            bad.append("forced register-staged kernel not taken")
        # the ping-pong forms: whole first tile in both directions (edge tiles are shifted, not clipped), two K-steps of the ring, a
        # token tile within two gate periods (the split-bf16 epilogues read the gate per row: launch_gemm_x3 has no such rule)
        kk = 3 * k if fl == X3 else k
        if kernel != FG_GEMM_REG and (rows < 256 or n < 256 or kk < (256 if fl == FP8 else 128) or (fl != X3 and gate_rows and gate_rows < 256)):
            bad.append("ping-pong form outside its envelope")
        if lds > 163840 or lds <= 0:
            bad.append("LDS")
        if not 1 <= grid <= cus:
            bad.append("grid")
        Mt, Nt = (rows + 255) // 256, (n + tile_n - 1) // tile_n
        if xn not in (0, 1, 2, 4, 8) or (xn > 0 and (grid % 8 or Nt % xn)):
            bad.append("xn")
        if (ks > 1) != (kernel == FG_GEMM_PP_SPLITK) or ks < 1:
            bad.append("ksplit and kernel form disagree")
        if ks > 1 and (heads or (k // 64) % ks or k // 64 // ks < 8 or Mt * Nt * ks > cus or ks * m * n * 4 > scratch):
            bad.append("split-K outside its rules")
        if not walk_is_exact(rows, n, tile_n, ks, xn, grid):
            bad.append("tile walk")
    if row != m:
        bad.append("pieces do not add up to m")
    return bad


MS = (1, 77, 255, 256, 257, 300, 513, 1000, 1300, 2048, 4680, 65536, 1200000)
NS = (16, 64, 128, 192, 256, 384, 400, 512, 1152, 1536, 3456, 4608, 8960)
KS = (64, 128, 256, 1152, 1536, 8960)
ORDERS = (0, 1, 2, 4, 8, 16 + 1, 32 + 1, 256 + 1, 64 + 1, 64 + 32 + 1)


@pytest.mark.parametrize("fl", [BF16, X3, FP8])
@pytest.mark.parametrize("cus", [64, 256, 304])
def test_plan_sweep(fl, cus):
    bad = {}
    for m, n, k in itertools.product(MS, NS, KS):
        for heads, gate_rows, scratch, order in itertools.product((0, 16), (0, 100, 256, 300, 1560), (0, 16 * m * n), ORDERS):
            v = violations(fl, m, n, k, heads, gate_rows, scratch, order, 0, cus)
            if v:
                bad.setdefault((m, n, k), set()).update(v)
    assert not bad, bad


@pytest.mark.parametrize("fl", [BF16, X3])
def test_plan_sweep_other_out_mode(fl):
    """out_mode 1 (bf16: fp32 out, the ping-pong kernel alone; split-bf16: [hi | lo] planes) over the same shapes."""
    bad = {}
    for m, n, k in itertools.product(MS, NS, KS):
        for heads, gate_rows, order, cus in itertools.product((0, 16), (0, 100, 256), (1, 2, 16 + 1, 32 + 1, 256 + 1), (64, 256)):
            v = violations(fl, m, n, k, heads, gate_rows, 0, order, 1, cus)
            if v:
                bad.setdefault((m, n, k), set()).update(v)
    assert not bad, bad


REG, PP, NARROW, SPLITK = FG_GEMM_REG, FG_GEMM_PP, FG_GEMM_PP_NARROW, FG_GEMM_PP_SPLITK
TOK, HEADS, RAW, TOK32 = FG_GEMM_EPI_TOK, FG_GEMM_EPI_HEADS, FG_GEMM_EPI_RAW, FG_GEMM_EPI_TOK32
# (flavour, m, n, k, options) -> (kernel, tile_n, epilogue, ksplit, grid, xn) at 256 CUs, tile_order 1 unless stated: the DiT-XL/2 and
# video-DiT block linears and the shapes of tests/test_gemm.py, as the launchers before gemm_plan decided them
ANCHORS = [
    ((BF16, 65536, 3456, 1152, dict(heads=16)), (PP, 256, HEADS, 1, 256, 2)),
    ((BF16, 65536, 1152, 1152, dict(gate_rows=256)), (PP, 256, TOK, 1, 256, 1)),
    ((BF16, 65536, 4608, 1152, {}), (PP, 256, TOK, 1, 256, 2)),
    ((BF16, 4680, 1536, 1536, dict(gate_rows=1560)), (NARROW, 128, TOK, 1, 228, 0)),
    ((BF16, 4680, 1536, 1536, dict(gate_rows=1560, order=32 + 1, scratch=16 * 4680 * 1536)), (SPLITK, 256, RAW, 2, 228, 0)),
    ((BF16, 4680, 1536, 8960, dict(scratch=16 * 4680 * 1536)), (NARROW, 128, TOK, 1, 228, 0)),
    ((BF16, 4680, 4608, 1536, {}), (NARROW, 128, TOK, 1, 256, 4)),
    ((BF16, 4680, 8960, 1536, {}), (PP, 256, TOK, 1, 256, 1)),
    ((BF16, 1000, 512, 2048, dict(order=32 + 1, scratch=16 * 1000 * 512)), (SPLITK, 256, RAW, 4, 32, 0)),
    ((BF16, 256, 256, 1024, dict(order=32 + 1, scratch=16 * 256 * 256)), (SPLITK, 256, RAW, 2, 2, 0)),
    ((BF16, 256, 256, 64, {}), (REG, 256, TOK, 1, 1, 0)),
    ((BF16, 512, 192, 128, {}), (REG, 192, TOK, 1, 2, 0)),
    ((BF16, 77, 3456, 1152, {}), (REG, 192, TOK, 1, 18, 0)),
    ((BF16, 513, 384, 384, {}), (NARROW, 128, TOK, 1, 9, 0)),
    ((BF16, 513, 384, 384, dict(order=32 + 1)), (PP, 256, TOK, 1, 6, 0)),
    ((BF16, 1000, 1152, 1152, dict(order=16 + 1)), (REG, 192, TOK, 1, 24, 0)),
    ((BF16, 2048, 4608, 1152, {}), (PP, 256, TOK, 1, 144, 0)),
    ((BF16, 1300, 1152, 1152, dict(gate_rows=100)), (REG, 192, TOK, 1, 36, 0)),
    ((BF16, 1000, 1152, 1152, dict(out_mode=1)), (PP, 256, TOK32, 1, 20, 0)),
    ((FP8, 65536, 3456, 1152, dict(heads=16)), (PP, 256, HEADS, 1, 256, 2)),
    ((FP8, 513, 384, 128, {}), (REG, 192, TOK, 1, 6, 0)),
]


@pytest.mark.parametrize("i", range(len(ANCHORS)))
def test_named_shapes_keep_their_plans(i):
    """A change of the rules cannot silently move the engines' shapes, or the GPU tests', to another kernel, grid or tile order."""
    (fl, m, n, k, opt), want = ANCHORS[i]
    p = dict(zip(FIELDS, plan(fl, m, n, k, **opt)))
    assert p["refusal"] == 0 and (p["pieces"], p["row0"], p["rows"]) == (1, 0, m)
    assert (p["kernel"], p["tile_n"], p["epilogue"], p["ksplit"], p["grid"], p["xn"]) == want


def test_named_refusals_and_row_pieces():
    assert plan(BF16, 100, 1152, 1152, out_mode=1)[0] == FG_GEMM_REFUSE_FORM  # fp32 out below one ping-pong tile
    assert plan(FP8, 300, 3456, 128, heads=16)[0] == FG_GEMM_REFUSE_FORM      # the fp8 head split at k < 256
    # 1 200 000 tokens x 1152 x 1152 in bf16: two launches, 931 840 + 268 160 rows
    for piece, (row0, rows) in enumerate(((0, 931840), (931840, 268160))):
        p = dict(zip(FIELDS, plan(BF16, 1200000, 1152, 1152, piece=piece)))
        assert (p["refusal"], p["pieces"], p["row0"], p["rows"]) == (0, 2, row0, rows)
        assert (p["kernel"], p["tile_n"], p["epilogue"], p["ksplit"], p["grid"], p["xn"]) == (PP, 256, TOK, 1, 256, 1)
    assert plan(BF16, 1200000, 1152, 1152, piece=2)[0] == FG_GEMM_REFUSE_ARG
    # the 2 GiB limits: W, and a shape so wide that not one 256-row tile of out stays below it
    assert plan(BF16, 256, 1 << 14, 1 << 16)[0] == FG_GEMM_REFUSE_OFFSET and plan(BF16, 256, 1 << 14, (1 << 16) - 64)[0] == 0
    assert plan(X3, 512, 4096, 87424)[0] == FG_GEMM_REFUSE_OFFSET
    assert plan(BF16, 256, 1 << 23, 64)[0] == FG_GEMM_REFUSE_OFFSET
    assert plan(X3, 116480 + 128, 1152, 4608)[0] == FG_GEMM_REFUSE_PIECE and plan(X3, 116480 + 256, 1152, 4608)[0] == 0
    # bad arguments: counts, granules, heads that do not divide n, bits and modes the flavour does not take, the CU count
    for fl, kw in ((BF16, dict(m=0)), (BF16, dict(n=-16)), (BF16, dict(k=96)), (BF16, dict(n=1160)), (BF16, dict(heads=7)), (BF16, dict(order=512 + 1)),
                   (BF16, dict(order=512)), (BF16, dict(order=16 + 32)), (BF16, dict(order=256 + 32)), (BF16, dict(order=128)), (BF16, dict(order=1024)),
                   (BF16, dict(order=-1)), (BF16, dict(out_mode=2)), (BF16, dict(cus=0)), (BF16, dict(gate_rows=-1)), (BF16, dict(piece=-1)),
                   (FP8, dict(k=1152 + 64)), (FP8, dict(order=32 + 1)), (FP8, dict(out_mode=1)), (X3, dict(m=255)), (X3, dict(n=240)),
                   (X3, dict(order=16 + 1)), (X3, dict(heads=32)), (3, {}), (-1, {})):
        a = dict(m=512, n=1152, k=1152)
        a.update(kw)
        assert plan(fl, **a) == (FG_GEMM_REFUSE_ARG,) + (0,) * 10, (fl, kw)
