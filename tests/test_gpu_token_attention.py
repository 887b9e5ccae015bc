"""Token attention (wan.hip fa_kernel<128|72>, fa2_kernel, fa72_seq_kernel, fa128_combine_kernel behind launch_fa), every kernel form
and launch path per ELEMENT against fp64 softmax attention of the same bf16 operands: |got - want| <= bound() of
tests/token_attention_ref.py, whose derivation is in its docstring.  The inputs are structured so that a subtly wrong kernel cannot
stay inside the bound; the unmarked tests below prove that on the CPU by applying each defect to the reference itself."""
import ctypes
import functools

import pytest
import torch

from fastgen_amd import _lib
from fastgen_amd._lib import (FG_FA_SEQ72, FG_FA_TILE72, FG_FA_TILE72_W3, FG_FA_TILE128, FG_FA_TILE128_REG, FG_FA_TILE128_W3, FG_FA_WIDE,
                              FG_FA_WIDE_CUT)

import token_attention_ref as TR

FORM = {FG_FA_TILE128: "fa_kernel<128,2,dma>", FG_FA_TILE128_W3: "fa_kernel<128,3,dma>", FG_FA_TILE128_REG: "fa_kernel<128,2,reg>",
        FG_FA_WIDE: "fa2_kernel even", FG_FA_WIDE_CUT: "fa2_kernel cut", FG_FA_SEQ72: "fa72_seq_kernel", FG_FA_TILE72: "fa_kernel<72,2>",
        FG_FA_TILE72_W3: "fa_kernel<72,3>"}


class Case:
    """One launch: the shape, the switches and what the plan must say about it (kernel form, splits, cut, sample-major map)."""

    def __init__(self, hd, B, H, Lq, Lkv, path, expect, fs=0, scratch=1):
        self.hd, self.B, self.H, self.Lq, self.Lkv, self.path, self.fs, self.scratch, self.expect = hd, B, H, Lq, Lkv, path, fs, scratch, expect

    def __repr__(self):
        return "hd%d-%dx%dx%dx%d-path%d-fs%d" % (self.hd, self.B, self.H, self.Lq, self.Lkv, self.path, self.fs)

    def plan(self):
        p = _lib.fg_attention_plan()
        assert _lib.lib().fg_op_attention_plan(self.hd, self.B, self.H, self.Lq, self.Lkv, self.H * self.hd, self.scratch, self.fs, self.path,
                                               ctypes.byref(p)) == 0
        return p

    def pieces(self):
        """key tiles [t0, nt) per split: the kernels' expressions (see tests/test_token_attention_plan.py pieces())"""
        p, nt = self.plan(), (self.Lkv + 31) // 32
        if p.t_cut:
            return [(0, p.t_cut), (p.t_cut, nt)]
        return [(s * nt // p.nsplit, (s + 1) * nt // p.nsplit) for s in range(p.nsplit)]


def _tile128(path):
    K = path
    return [Case(128, 2, 3, 200, 333, path, (K, 1, 0, 0)), Case(128, 1, 2, 48, 17, path, (K, 1, 0, 0)),
            Case(128, 1, 2, 130, 64, path, (K, 1, 0, 0)), Case(128, 9, 2, 100, 77, path, (K, 1, 0, 1)),
            Case(128, 1, 2, 200, 100, path, (K, 4, 0, 0), fs=8)]  # (4 key tiles: a forced split of 8 clamps to them)


SELECTION = (
    _tile128(FG_FA_TILE128) + _tile128(FG_FA_TILE128_W3) + _tile128(FG_FA_TILE128_REG)
    + [Case(128, 1, 2, 200, 333, FG_FA_TILE128, (FG_FA_TILE128, n, 0, 0), fs=n) for n in range(1, 9)]
    + [Case(128, 1, 2, 200, 333, FG_FA_TILE128_W3, (FG_FA_TILE128_W3, 3, 0, 0), fs=3),
       Case(128, 1, 2, 200, 333, FG_FA_TILE128_REG, (FG_FA_TILE128_REG, 8, 0, 0), fs=8),
       # fa2_kernel: the launcher's own choice from 1024 keys (the cut), forced even splits over 33 tiles, the cost model's even split
       Case(128, 1, 2, 300, 1037, 0, (FG_FA_WIDE_CUT, 2, 17, 0)), Case(128, 2, 3, 257, 1024, 0, (FG_FA_WIDE_CUT, 2, 16, 0)),
       Case(128, 1, 2, 300, 1037, 0, (FG_FA_WIDE, 1, 0, 0), fs=1), Case(128, 1, 2, 300, 1037, 0, (FG_FA_WIDE, 3, 0, 0), fs=3),
       Case(128, 1, 2, 300, 1037, 0, (FG_FA_WIDE, 8, 0, 0), fs=8), Case(128, 1, 2, 300, 1037, FG_FA_WIDE, (FG_FA_WIDE, 4, 0, 0)),
       # ... on short key counts: one ragged tile; one tile per split
       Case(128, 1, 2, 100, 17, FG_FA_WIDE, (FG_FA_WIDE, 1, 0, 0)), Case(128, 1, 2, 100, 96, FG_FA_WIDE, (FG_FA_WIDE, 3, 0, 0), fs=3),
       # ... the cut in the middle, with a one-tile short piece, with the ragged tile alone as the short piece, and where the rule
       # used to put it past the keys (209 pieces, 32 key tiles)
       Case(128, 1, 100, 64, 1100, 0, (FG_FA_WIDE_CUT, 2, 18, 0)), Case(128, 1, 208, 64, 1024, 0, (FG_FA_WIDE_CUT, 2, 31, 0)),
       Case(128, 1, 208, 64, 1000, FG_FA_WIDE_CUT, (FG_FA_WIDE_CUT, 2, 31, 0)), Case(128, 1, 209, 64, 1024, 0, (FG_FA_WIDE_CUT, 2, 31, 0)),
       Case(128, 1, 209, 64, 1000, FG_FA_WIDE_CUT, (FG_FA_WIDE_CUT, 2, 31, 0)),
       # head dim 72
       Case(72, 3, 16, 256, 256, 0, (FG_FA_SEQ72, 1, 0, 1)), Case(72, 1, 2, 100, 77, FG_FA_SEQ72, (FG_FA_SEQ72, 1, 0, 1)),
       Case(72, 2, 4, 300, 250, 0, (FG_FA_SEQ72, 1, 0, 1)), Case(72, 9, 2, 129, 1, 0, (FG_FA_SEQ72, 1, 0, 1))]
    + [c for K in (FG_FA_TILE72, FG_FA_TILE72_W3) for c in (
        Case(72, 2, 4, 300, 1000, K, (K, 4, 0, 0)), Case(72, 2, 4, 300, 250, K, (K, 3, 0, 0), fs=3), Case(72, 9, 2, 100, 300, K, (K, 1, 0, 1)),
        Case(72, 1, 2, 100, 77, K, (K, 1, 0, 0)))])

# a ragged (or exactly full) last key tile per form: Lkv % 32 in {1, 17, 31, 0} and fewer than 32 keys; fa72_seq_kernel: {1, 77, 255, 256}
PADDING = (
    [Case(128, 1, 2, 130, Lkv, K, (K, 1, 0, 0)) for K in (FG_FA_TILE128, FG_FA_TILE128_W3, FG_FA_TILE128_REG, FG_FA_WIDE) for Lkv in (17, 33, 49, 63, 64)]
    + [Case(128, 1, 2, 130, 97, FG_FA_TILE128, (FG_FA_TILE128, 4, 0, 0), fs=4), Case(128, 1, 2, 130, 97, FG_FA_WIDE, (FG_FA_WIDE, 4, 0, 0), fs=4),
       Case(128, 1, 2, 300, 1025, 0, (FG_FA_WIDE_CUT, 2, 17, 0)), Case(128, 1, 2, 300, 1041, 0, (FG_FA_WIDE_CUT, 2, 17, 0)),
       Case(128, 1, 2, 300, 1055, 0, (FG_FA_WIDE_CUT, 2, 17, 0)), Case(128, 1, 208, 64, 1000, FG_FA_WIDE_CUT, (FG_FA_WIDE_CUT, 2, 31, 0)),
       Case(128, 1, 209, 64, 1000, FG_FA_WIDE_CUT, (FG_FA_WIDE_CUT, 2, 31, 0)), Case(128, 1, 209, 64, 1024, 0, (FG_FA_WIDE_CUT, 2, 31, 0))]
    + [Case(72, 2, 3, 130, Lkv, 0, (FG_FA_SEQ72, 1, 0, 1)) for Lkv in (1, 77, 255, 256)]
    + [Case(72, 1, 2, 130, Lkv, K, (K, 1, 0, 0)) for K in (FG_FA_TILE72, FG_FA_TILE72_W3) for Lkv in (17, 33, 49, 63, 64)])

# one case per kernel form for the poisoned layouts
LAYOUT_CASES = [Case(128, 2, 3, 200, 333, K, (K, 1, 0, 0)) for K in (FG_FA_TILE128, FG_FA_TILE128_W3, FG_FA_TILE128_REG)] + [
    Case(128, 2, 2, 200, 333, FG_FA_TILE128, (FG_FA_TILE128, 3, 0, 0), fs=3), Case(128, 9, 2, 100, 77, FG_FA_TILE128, (FG_FA_TILE128, 1, 0, 1)),
    Case(128, 2, 2, 257, 1037, 0, (FG_FA_WIDE_CUT, 2, 17, 0)), Case(128, 2, 2, 257, 1037, 0, (FG_FA_WIDE, 3, 0, 0), fs=3),
    Case(72, 2, 4, 300, 250, 0, (FG_FA_SEQ72, 1, 0, 1)), Case(72, 2, 4, 300, 250, FG_FA_TILE72, (FG_FA_TILE72, 3, 0, 0), fs=3),
    Case(72, 2, 4, 300, 333, FG_FA_TILE72_W3, (FG_FA_TILE72_W3, 1, 0, 0), scratch=0)]
LAYOUTS = ("packed_qkv", "interleaved_kv", "cache")


def test_every_form_is_served():
    """every kernel form has a selection, a padding-leak and a poisoned-layout case, and every case names the form the plan gives it"""
    for cases in (SELECTION, PADDING, LAYOUT_CASES):
        assert {c.expect[0] for c in cases} == set(FORM)
        for c in cases:
            p = c.plan()
            assert p.refusal == 0 and (p.kernel, p.nsplit, p.t_cut, p.sample_major) == c.expect, c


# ---- the inputs reject wrong kernels (CPU) ------------------------------------------------------------------------------------------
def _violates(mut, ref, bnd):
    return bool(((mut - ref["want"]).abs() > bnd).any())


@pytest.mark.parametrize("c", [Case(128, 1, 2, 200, 333, FG_FA_TILE128, None, fs=3), Case(128, 1, 2, 48, 17, FG_FA_TILE128, None),
                               Case(128, 1, 2, 300, 1037, 0, None), Case(128, 1, 2, 100, 96, FG_FA_WIDE, None, fs=3),
                               Case(72, 1, 2, 100, 77, FG_FA_SEQ72, None), Case(72, 2, 4, 300, 250, FG_FA_TILE72, None, fs=3)], ids=repr)
def test_selection_input_rejects_its_mutations(c):
    """last key dropped, two keys of a tile swapped (head dim 72: twins that differ in dims 64 .. 67 only), a query row shifted, each
    split's partial dropped: every one leaves the bound somewhere; the reference rounded to bf16 stays inside (it IS v[pi])."""
    q, k, v, pi = TR.selection(c.B, c.H, c.hd, c.Lq, c.Lkv, c.pieces())
    ref = TR.reference(q, k, v, c.H, c.hd)
    bnd = TR.bound(ref, c.hd, c.Lkv, float(v.float().abs().max()))
    assert float(ref["lead"].min()) > 40.0
    assert set(TR.edge_keys(c.Lkv, c.pieces())) <= set(pi.flatten().tolist())
    rounded = TR.round_bf16(ref["want"])
    assert not _violates(rounded.double(), ref, bnd)
    picked = torch.gather(v.view(c.B, c.Lkv, c.H, c.hd).permute(0, 2, 1, 3), 2, pi[..., None].expand(-1, -1, -1, c.hd))
    assert torch.equal(rounded.view(c.B, c.Lq, c.H, c.hd).permute(0, 2, 1, 3), picked)
    muts = [("drop_last", None), ("shift_row", 0), ("shift_row", c.Lq - 2), ("swap_keys", 0), ("swap_keys", (c.Lkv - 2) & ~1)]
    muts += [("drop_piece", pc) for pc in c.pieces()] if len(c.pieces()) > 1 else []
    for name, arg in muts:
        assert _violates(TR.mutate(name, q, k, v, c.H, c.hd, arg), ref, bnd), (name, arg)


@pytest.mark.parametrize("hd,Lkv", [(128, 17), (128, 33), (128, 63), (128, 64), (128, 1000), (72, 1), (72, 77), (72, 255), (72, 256)])
def test_padding_input_rejects_a_phantom_key(hd, Lkv):
    """one zero key appended (an unmasked padding row) leaves the bound; the largest real score is 20 bits below zero"""
    B, H, Lq = 1, 2, 130
    q, k, v = TR.padding_leak(B, H, hd, Lq, Lkv)
    ref = TR.reference(q, k, v, H, hd)
    bnd = TR.bound(ref, hd, Lkv, float(v.float().abs().max()))
    assert float(ref["top"].max()) < -20.0
    assert not _violates(TR.round_bf16(ref["want"]).double(), ref, bnd)
    assert _violates(TR.mutate("zero_key", q, k, v, H, hd), ref, bnd)


@pytest.mark.parametrize("order", ["rising", "falling", "spikes"])
def test_moving_maxima_input_rejects_its_mutations(order):
    """a query row shifted, and the heaviest split's partial dropped from the merge (3 and 8 even splits, the cut at tile 17)"""
    B, H, hd, Lq, Lkv = 1, 2, 128, 300, 1037
    q, k, v = TR.moving_maxima(order, B, H, hd, Lq, Lkv)
    ref = TR.reference(q, k, v, H, hd)
    bnd = TR.bound(ref, hd, Lkv, float(v.float().abs().max()))
    assert not _violates(TR.round_bf16(ref["want"]).double(), ref, bnd)
    assert _violates(TR.mutate("shift_row", q, k, v, H, hd, 7), ref, bnd)
    heavy = {"rising": -1, "falling": 0, "spikes": 0}[order]
    for pcs in ([(s * 33 // 3, (s + 1) * 33 // 3) for s in range(3)], [(s * 33 // 8, (s + 1) * 33 // 8) for s in range(8)], [(0, 17), (17, 33)]):
        assert _violates(TR.mutate("drop_piece", q, k, v, H, hd, pcs[heavy]), ref, bnd), pcs[heavy]


# ---- the kernels (GPU) ----------------------------------------------------------------------------------------------------------------
HEADROOM = {}


@pytest.fixture(scope="module", autouse=True)
def _headroom_table():
    yield
    for form in sorted(HEADROOM):
        print("\nheadroom %-22s max err / (2^-9 A) = %.3f" % (form, HEADROOM[form]), end="")


def _run(c, q, ldq, q_bs, k, v, ldk, kv_bs, out, ldo, o_bs):
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().fg_op_attention_ex(p(q), ldq, q_bs, p(k), p(v), ldk, kv_bs, p(out), ldo, o_bs, c.B, c.H, c.hd, c.Lq, c.Lkv, c.scratch,
                                             c.fs, c.path, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


def _run_plain(c, q, k, v):
    D = c.H * c.hd
    q, k, v = q.cuda(), k.cuda(), v.cuda()
    out = torch.full_like(q, float("nan"))
    _run(c, q, D, c.Lq * D, k, v, D, c.Lkv * D, out, D, c.Lq * D)
    return out


def _check(c, got, q, k, v, what):
    """per element against the fp64 reference (computed on the GPU); records the headroom of the case's kernel form"""
    p = c.plan()
    assert p.refusal == 0 and (p.kernel, p.nsplit, p.t_cut, p.sample_major) == c.expect  # it ran on the form it names
    ref = TR.reference(q.cuda(), k.cuda(), v.cuda(), c.H, c.hd)
    bnd = TR.bound(ref, c.hd, c.Lkv, float(v.float().abs().max()))
    h = TR.headroom(got, ref)
    print("%s %r %s: max err / (2^-9 A) = %.3f" % (what, c, FORM[p.kernel], h))
    HEADROOM[FORM[p.kernel]] = max(HEADROOM.get(FORM[p.kernel], 0.0), h)
    err = (got.double() - ref["want"]).abs()
    assert bool(torch.isfinite(got.float()).all())
    worst = (err - bnd).max()
    assert bool((err <= bnd).all()), (c, what, float(worst), h)
    return ref


@functools.lru_cache(maxsize=None)
def _selection(hd, B, H, Lq, Lkv, pieces):
    return TR.selection(B, H, hd, Lq, Lkv, list(pieces))


@pytest.mark.gpu
@pytest.mark.parametrize("c", SELECTION, ids=repr)
def test_selection(c):
    """out[i] must be v[pi(i)] bit for bit: key 0, the last key of a ragged tile, both sides of every split boundary and of the cut,
    all rows of an even and an odd key tile, every query row of every query tile"""
    q, k, v, pi = _selection(c.hd, c.B, c.H, c.Lq, c.Lkv, tuple(c.pieces()))
    got = _run_plain(c, q, k, v)
    ref = _check(c, got, q, k, v, "selection")
    assert float(ref["lead"].min()) > 40.0
    picked = torch.gather(v.view(c.B, c.Lkv, c.H, c.hd).permute(0, 2, 1, 3), 2, pi[..., None].expand(-1, -1, -1, c.hd))
    assert torch.equal(got.cpu().view(c.B, c.Lq, c.H, c.hd).permute(0, 2, 1, 3), picked)


@pytest.mark.gpu
@pytest.mark.parametrize("c", PADDING, ids=repr)
def test_padding_leak(c):
    q, k, v = TR.padding_leak(c.B, c.H, c.hd, c.Lq, c.Lkv)
    ref = _check(c, _run_plain(c, q, k, v), q, k, v, "padding")
    assert float(ref["top"].max()) < -20.0


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["rising", "falling", "spikes"])
def test_moving_maxima(order):
    """fa2_kernel's eras under the per-element bound: one split, 3 and 8 even splits, the cut.  Scores reach hundreds of bits here, so
    the fp32 score accumulation is a visible share of the error (and of the bound), on either kernel."""
    B, H, hd, Lq, Lkv = 1, 2, 128, 300, 1037
    q, k, v = TR.moving_maxima(order, B, H, hd, Lq, Lkv)
    for fs, expect in ((1, (FG_FA_WIDE, 1, 0, 0)), (3, (FG_FA_WIDE, 3, 0, 0)), (8, (FG_FA_WIDE, 8, 0, 0)), (0, (FG_FA_WIDE_CUT, 2, 17, 0))):
        c = Case(hd, B, H, Lq, Lkv, 0, expect, fs=fs)
        _check(c, _run_plain(c, q, k, v), q, k, v, "maxima-" + order)
    # (fa_kernel's per-tile running maximum on the same scores, for the record of what the arithmetic alone costs at this magnitude)
    c = Case(hd, B, H, Lq, Lkv, FG_FA_TILE128, (FG_FA_TILE128, 1, 0, 0), fs=1)
    _check(c, _run_plain(c, q, k, v), q, k, v, "maxima-" + order)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("c", LAYOUT_CASES, ids=repr)
def test_poisoned_layouts(c, layout):
    """The engines' layouts with NaN wherever a kernel has no business reading - stale cache rows behind the last valid key, the
    gaps between samples, query rows behind Lq - and a sentinel wherever it has none writing: a row pitch above heads * hd and
    spare rows in `out`, which must come back bit-identical."""
    B, H, hd, Lq, Lkv, D = c.B, c.H, c.hd, c.Lq, c.Lkv, c.H * c.hd
    q, k, v, pi = _selection(hd, B, H, Lq, Lkv, tuple(c.pieces()))
    nan = float("nan")
    if layout == "packed_qkv":  # the DiT: rows q | k | v, ldq = ldk = 3 D, v = k + D
        rows = max(Lq, Lkv) + 5
        buf = torch.full((B, rows, 3 * D), nan, dtype=torch.bfloat16)
        buf[:, :Lq, :D], buf[:, :Lkv, D:2 * D], buf[:, :Lkv, 2 * D:] = q, k, v
        buf = buf.cuda()
        qb, kb, vb, ldq, q_bs, ldk, kv_bs = buf, buf[0, 0, D:], buf[0, 0, 2 * D:], 3 * D, rows * 3 * D, 3 * D, rows * 3 * D
    else:
        qb = torch.full((B, Lq + 3, D + 8), nan, dtype=torch.bfloat16)
        qb[:, :Lq, :D] = q
        qb, ldq, q_bs = qb.cuda(), D + 8, (Lq + 3) * (D + 8)
        if layout == "interleaved_kv":  # the video DiT's text cross-attention: rows k | v, ldk = 2 D
            kv = torch.full((B, Lkv + 7, 2 * D), nan, dtype=torch.bfloat16)
            kv[:, :Lkv, :D], kv[:, :Lkv, D:] = k, v
            kv = kv.cuda()
            kb, vb, ldk, kv_bs = kv, kv[0, 0, D:], 2 * D, (Lkv + 7) * 2 * D
        else:  # a partly filled KV cache: stale rows behind Lkv, a batch stride above Lkv * ldk
            cap = Lkv + 40
            kb, vb = torch.full((B, cap, D), nan, dtype=torch.bfloat16), torch.full((B, cap, D), nan, dtype=torch.bfloat16)
            kb[:, :Lkv], vb[:, :Lkv] = k, v
            kb, vb, ldk, kv_bs = kb.cuda(), vb.cuda(), D, cap * D
    sentinel = torch.tensor(-1234.0, dtype=torch.bfloat16)
    out = torch.full((B, Lq + 3, D + 8), float(sentinel), dtype=torch.bfloat16).cuda()
    _run(c, qb, ldq, q_bs, kb, vb, ldk, kv_bs, out, D + 8, (Lq + 3) * (D + 8))
    got = out[:, :Lq, :D].contiguous()
    _check(c, got, q, k, v, layout)
    picked = torch.gather(v.view(B, Lkv, H, hd).permute(0, 2, 1, 3), 2, pi[..., None].expand(-1, -1, -1, hd))
    assert torch.equal(got.cpu().view(B, Lq, H, hd).permute(0, 2, 1, 3), picked)
    out[:, :Lq, :D] = sentinel
    assert bool((out == sentinel).all())  # (no NaN sentinel: -1234 compares bit for bit)
