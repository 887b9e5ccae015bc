"""CPU-only sweep of token attention's launch plan (wan.hip fa_plan through fg_op_attention_plan): for every shape, scratch setting,
forced split and kernel form the plan must describe a launch in which every workgroup has keys to walk and every (sample, head,
query tile, split) has a workgroup.  Nothing is launched; no GPU is needed."""
import ctypes

import pytest

from fastgen_amd import _lib
from fastgen_amd._lib import (FG_FA_REFUSE_ARG, FG_FA_REFUSE_OFFSET, FG_FA_REFUSE_PATH, FG_FA_SEQ72, FG_FA_TILE72, FG_FA_TILE72_W3,
                              FG_FA_TILE128, FG_FA_TILE128_REG, FG_FA_TILE128_W3, FG_FA_WIDE, FG_FA_WIDE_CUT)

FA_MAX_SPLIT = 8
PATHS = {128: (0, FG_FA_TILE128, FG_FA_TILE128_W3, FG_FA_TILE128_REG, FG_FA_WIDE, FG_FA_WIDE_CUT),
         72: (0, FG_FA_SEQ72, FG_FA_TILE72, FG_FA_TILE72_W3)}
QUERY_TILE = {FG_FA_TILE128: 128, FG_FA_TILE128_W3: 128, FG_FA_TILE128_REG: 128, FG_FA_WIDE: 256, FG_FA_WIDE_CUT: 256, FG_FA_SEQ72: 128,
              FG_FA_TILE72: 128, FG_FA_TILE72_W3: 128}


def plan(hd, B, H, Lq, Lkv, ldk=None, scratch=1, force_split=0, path=0):
    p = _lib.fg_attention_plan()
    rc = _lib.lib().fg_op_attention_plan(hd, B, H, Lq, Lkv, H * hd if ldk is None else ldk, scratch, force_split, path, ctypes.byref(p))
    assert rc == 0
    return p


def pieces(p, Lkv):
    """The key tiles [t0, nt) each split's workgroups walk.  These are the kernels' own integer expressions: fa_kernel's and fa2_kernel's
    `t0 = split * ntiles / nsplit, nt = (split + 1) * ntiles / nsplit`, fa2_kernel's `t_cut > 0 ? (split ? t_cut : 0)` /
    `(split ? ntiles : t_cut)`; fa72_seq_kernel walks all of its (at most 8) tiles in one piece."""
    ntiles = (Lkv + 31) // 32
    if p.kernel == FG_FA_SEQ72:
        return [(0, ntiles)]
    if p.t_cut > 0:
        return [((p.t_cut if split else 0), (ntiles if split else p.t_cut)) for split in range(p.nsplit)]
    return [(split * ntiles // p.nsplit, (split + 1) * ntiles // p.nsplit) for split in range(p.nsplit)]


def model(hd, B, H, Lq, Lkv, scratch, force_split):
    """The launcher's cost model and cut rule, written out a second time: (nsplit before the cut, the cut as the rule gives it before it
    is clamped, whether the rule applies).  The sweep holds the plan to it, so that a change of either shows up here."""
    qtiles, ktiles = (Lq + 127) // 128, (Lkv + 31) // 32
    nsplit = 1
    if force_split > 0:
        nsplit = min(force_split, ktiles)
    elif scratch:
        best = -1.0
        for c in range(1, FA_MAX_SPLIT + 1):
            if c > 1 and ktiles // c < 8:
                break
            per_cu = ((B * H * c + 7) // 8 * qtiles + 31) // 32
            cost = 0.5 * float(per_cu) * ((ktiles + c - 1) // c + 6) + (3.0 + 6.7e-7 * c * B * float(Lq) * H * hd if c > 1 else 0.0)
            if best < 0.0 or cost < best:
                best, nsplit = cost, c
    P = B * H * ((Lq + 255) // 256)
    t_cut = 0
    if hd == 128 and force_split == 0 and scratch and P <= 248 and ktiles >= 32:
        f = float(P) * (ktiles + 6) / (float(ktiles) * 256.0)
        if f < 0.97:
            t_cut = max(int(f * ktiles) + 1, (ktiles + 1) // 2)
    return nsplit, t_cut


def violations(hd, B, H, Lq, Lkv, scratch, force_split, path):
    """The names of the invariants this plan breaks (empty: none)."""
    p = plan(hd, B, H, Lq, Lkv, None, scratch, force_split, path)
    bad = []
    ktiles = (Lkv + 31) // 32
    if force_split > 1 and not scratch:
        return [] if p.refusal == FG_FA_REFUSE_ARG else ["a forced split without scratch is not refused"]
    if (hd == 128 and Lkv * H * hd * 2 >= 1 << 31) or p.refusal == FG_FA_REFUSE_OFFSET:  # (32-bit buffer offsets; ldk = H * hd here)
        return [] if (hd == 128 and Lkv * H * hd * 2 >= 1 << 31) and p.refusal == FG_FA_REFUSE_OFFSET else ["offset guard moved"]
    if p.refusal:
        if p.refusal != FG_FA_REFUSE_PATH or path == 0:
            return ["refusal %d" % p.refusal]
        # a refused form is one the launcher's rules do not arrive at under that form's switches - never a redirection
        own = plan(hd, B, H, Lq, Lkv, None, scratch, force_split, 0)
        if path == own.kernel:
            bad.append("the launcher's own form is refused when named")
        return bad
    if path and p.kernel != path:
        bad.append("another form than the one named")
    if p.kernel not in PATHS[hd][1:]:
        bad.append("kernel form of the other head dim")
    # every piece of every split holds at least one key tile, and the pieces tile [0, ktiles)
    pc = pieces(p, Lkv)
    if any(nt - t0 < 1 for t0, nt in pc):
        bad.append("empty key piece")
    if pc[0][0] != 0 or pc[-1][1] != ktiles or any(a[1] != b[0] for a, b in zip(pc[:-1], pc[1:])):
        bad.append("pieces do not tile the keys")
    if (p.kernel == FG_FA_WIDE_CUT) != (p.t_cut > 0):
        bad.append("cut and kernel form disagree")
    if p.t_cut and not (0 < p.t_cut < ktiles and p.nsplit == 2 and scratch and force_split == 0):
        bad.append("cut out of range")
    if not 1 <= p.nsplit <= min(FA_MAX_SPLIT, ktiles):
        bad.append("nsplit out of range")
    if force_split and p.nsplit != min(force_split, ktiles):
        bad.append("forced split not taken")
    # partial outputs [nsplit][B Lq][H hd] fp32, their log-sum-exps [nsplit][B Lq][H] behind room for FA_MAX_SPLIT partial outputs
    if p.nsplit > 1 and (not scratch or p.scratch_bytes < 4 * (FA_MAX_SPLIT * B * Lq * H * hd + p.nsplit * B * Lq * H)):
        bad.append("split without (enough) scratch")
    if p.kernel == FG_FA_SEQ72 and Lkv > 256:
        bad.append("whole-sequence kernel over more than 256 keys")
    # the grid covers every unit under the kernel's own workgroup map
    qtiles = (Lq + QUERY_TILE[p.kernel] - 1) // QUERY_TILE[p.kernel]
    if p.sample_major:
        if p.nsplit != 1 or p.kernel in (FG_FA_WIDE, FG_FA_WIDE_CUT):
            bad.append("sample-major map with a split or fa2_kernel")
        if p.grid != (B + 7) // 8 * 8 * H * qtiles:  # workgroup (xcd, slot): sample (slot / qtiles / heads) * 8 + xcd
            bad.append("sample-major grid")
    elif p.t_cut:
        P, per = B * H * qtiles, (B * H * qtiles + 7) // 8  # XCD x runs pieces [x P / 8, (x + 1) P / 8) in `per` padded slots, twice
        if p.grid != 2 * 8 * per or any((x + 1) * P // 8 - x * P // 8 > per for x in range(8)):
            bad.append("cut grid")
    elif p.grid != (B * H * p.nsplit + 7) // 8 * 8 * qtiles:  # workgroup (xcd, slot): unit (slot / qtiles) * 8 + xcd
        bad.append("unit grid")
    if (p.sample_major != 0) != (p.kernel == FG_FA_SEQ72 or (p.nsplit == 1 and B >= 8 and Lq <= 1024 and p.kernel not in (FG_FA_WIDE, FG_FA_WIDE_CUT))):
        bad.append("sample-major rule moved")
    # the cost model's outputs stay where they were: the split count, and the cut wherever it left the short piece a tile
    if path == 0 or p.kernel == path:
        nsplit, t_cut = model(hd, B, H, Lq, Lkv, scratch, force_split)
        if p.kernel == FG_FA_WIDE_CUT:
            if p.t_cut != min(t_cut, ktiles - 1):
                bad.append("cut moved")
        elif p.nsplit != nsplit:
            bad.append("split count moved")
        if path == 0 and hd == 128 and Lkv >= 1024 and not p.sample_major and (p.kernel == FG_FA_WIDE_CUT) != (t_cut > 0):
            bad.append("cut rule moved")
    return bad


def _lkvs():
    out = set()
    for c in (32, 256, 1024, 4680, 32760):  # every residue mod 32 around each (1024: 992 .. 1056)
        out.update(range(max(1, c - 32), c + 33))
    return sorted(out)


def _shapes(P):
    """(B, heads, Lq) with B * heads * ceil(Lq / 256) = P: one query tile, a ragged second one, nine samples (the sample-major map)."""
    out = [(1, P, 64)]
    if P % 3 == 0:
        out.append((1, P // 3, 700))
    if P % 9 == 0:
        out.append((9, P // 9, 100))
    if P % 10 == 0:
        out.append((2, P // 10, 1100))
    return out


@pytest.mark.parametrize("hd", [128, 72])
def test_plan_sweep_every_piece_count(hd):
    """P = B * heads * query tiles from 1 to 600 at every key count of the list, under the launcher's own choice."""
    bad = {}
    for P in range(1, 601):
        for B, H, Lq in _shapes(P):
            for Lkv in _lkvs():
                v = violations(hd, B, H, Lq, Lkv, 1, 0, 0)
                if v:
                    bad.setdefault((P, (Lkv + 31) // 32), set()).update(v)
    assert not bad, bad


@pytest.mark.parametrize("hd", [128, 72])
def test_plan_sweep_every_switch(hd):
    """Scratch on and off, every forced split, every kernel form, at the piece counts and key counts where a rule changes."""
    bad = {}
    for P in (1, 2, 7, 8, 9, 16, 31, 63, 64, 65, 90, 207, 208, 209, 210, 247, 248, 249, 255, 256, 257, 512, 600):
        for B, H, Lq in _shapes(P):
            for Lkv in (1, 17, 31, 32, 33, 64, 100, 255, 256, 257, 288, 992, 993, 1000, 1023, 1024, 1025, 1037, 1056, 4680, 32737, 32760, 32768):
                for scratch in (0, 1):
                    for fs in range(FA_MAX_SPLIT + 1):
                        for path in PATHS[hd]:
                            v = violations(hd, B, H, Lq, Lkv, scratch, fs, path)
                            if v:
                                bad.setdefault((P, (Lkv + 31) // 32, scratch, fs, path), set()).update(v)
    assert not bad, bad


def test_the_one_cut_the_rule_put_past_the_keys():
    """f ktiles = P (ktiles + 6) / 256 reaches ktiles - 1 below f = 0.97 only at P = 209, ktiles = 32 (exhaustive over the rule's whole
    domain P <= 248, here up to 4000 key tiles): (int)(f ktiles) + 1 = ktiles left the short piece [32, 32).  The plan keeps it a tile."""
    hits = []
    for ktiles in range(32, 4000):
        for P in range(1, 249):
            f = float(P) * (ktiles + 6) / (float(ktiles) * 256.0)
            if f < 0.97 and max(int(f * ktiles) + 1, (ktiles + 1) // 2) >= ktiles:
                hits.append((P, ktiles))
    assert hits == [(209, 32)]
    for Lkv, path in ((993, FG_FA_WIDE_CUT), (1000, FG_FA_WIDE_CUT), (1024, FG_FA_WIDE_CUT), (1024, 0)):  # (below 1024 keys fa2_kernel is a choice)
        p = plan(128, 1, 209, 64, Lkv, path=path)
        assert (p.kernel, p.nsplit, p.t_cut, p.grid) == (FG_FA_WIDE_CUT, 2, 31, 2 * 8 * 27)


def test_refusals():
    big = 1 << 31
    # 32-bit buffer offsets (head dim 128): lkv * ldk * 2 bytes
    assert plan(128, 1, 12, 4680, 32760, ldk=32768).refusal == 0
    assert plan(128, 1, 12, 4680, 32768, ldk=32768).refusal == FG_FA_REFUSE_OFFSET
    assert plan(128, 1, 160, 64, 52429, ldk=20480).refusal == FG_FA_REFUSE_OFFSET and 52429 * 20480 * 2 >= big > 52428 * 20480 * 2
    assert plan(128, 1, 160, 64, 52428, ldk=20480).refusal == 0
    for path in PATHS[128][1:]:
        assert plan(128, 1, 12, 300, 32768, ldk=32768, path=path).refusal == FG_FA_REFUSE_OFFSET
    # bad arguments
    for kw in (dict(hd=64), dict(B=0), dict(H=0), dict(Lq=0), dict(Lkv=0), dict(ldk=260), dict(force_split=9), dict(force_split=-1),
               dict(force_split=2, scratch=0), dict(path=9), dict(path=-1)):
        a = dict(hd=128, B=1, H=2, Lq=100, Lkv=100, ldk=256, scratch=1, force_split=0, path=0)
        a.update(kw)
        p = plan(**a)
        assert (p.refusal, p.kernel, p.nsplit, p.grid, p.scratch_bytes) == (FG_FA_REFUSE_ARG, 0, 0, 0, 0), kw
    # forms that cannot serve a shape are refused, not redirected
    assert plan(72, 1, 2, 100, 257, path=FG_FA_SEQ72).refusal == FG_FA_REFUSE_PATH  # more than 256 keys
    assert plan(72, 1, 2, 100, 250, force_split=3, path=FG_FA_SEQ72).refusal == FG_FA_REFUSE_PATH  # it has no split form
    assert plan(128, 1, 100, 64, 1100, force_split=2, path=FG_FA_WIDE_CUT).refusal == FG_FA_REFUSE_PATH  # a cut with a forced split
    assert plan(128, 1, 100, 64, 1100, scratch=0, path=FG_FA_WIDE_CUT).refusal == FG_FA_REFUSE_PATH  # the cut needs the merge's scratch
    assert plan(128, 1, 100, 64, 992, path=FG_FA_WIDE_CUT).refusal == FG_FA_REFUSE_PATH  # fewer than 32 key tiles
    assert plan(128, 1, 249, 64, 1100, path=FG_FA_WIDE_CUT).refusal == FG_FA_REFUSE_PATH  # a workgroup per CU already
    assert plan(128, 9, 2, 100, 1100, scratch=0, path=FG_FA_WIDE).refusal == FG_FA_REFUSE_PATH  # the sample-major map is fa_kernel's
    assert plan(128, 1, 2, 100, 100, path=FG_FA_TILE72).refusal == FG_FA_REFUSE_PATH  # the other head dim
    assert plan(72, 1, 2, 100, 100, path=FG_FA_TILE128).refusal == FG_FA_REFUSE_PATH


# name: (head dim, B, heads, Lq, Lkv, ldk in units of heads * head dim, scratch, forced split, path) -> (kernel form, splits, cut, sample-major)
NAMED = {
    # the causal video DiT (12 heads x 128, 4680 tokens per chunk): self-attention over the KV cache of chunk 1, 4 and 7; text cross-attention
    "wan_self_chunk1": ((128, 1, 12, 4680, 4680, 1, 1, 0, 0), (FG_FA_WIDE_CUT, 2, 137, 0)),
    "wan_self_chunk4": ((128, 1, 12, 4680, 18720, 1, 1, 0, 0), (FG_FA_WIDE_CUT, 2, 527, 0)),
    "wan_self_chunk7": ((128, 1, 12, 4680, 32760, 1, 1, 0, 0), (FG_FA_WIDE_CUT, 2, 918, 0)),
    "wan_text_cross": ((128, 1, 12, 4680, 512, 2, 1, 0, 0), (FG_FA_TILE128, 1, 0, 0)),
    "wan_self_two_samples": ((128, 2, 12, 4680, 4680, 1, 1, 0, 0), (FG_FA_WIDE, 2, 0, 0)),
    # DiT-XL/2 (16 heads x 72, 256 tokens, packed q|k|v rows)
    "dit_xl2_b256": ((72, 256, 16, 256, 256, 3, 0, 0, 0), (FG_FA_SEQ72, 1, 0, 1)),
    "dit_xl2_b1": ((72, 1, 16, 256, 256, 3, 0, 0, 0), (FG_FA_SEQ72, 1, 0, 1)),
    # the shapes of tests/test_gpu_token_attention.py, under the launcher's own choice
    "tile128_ragged": ((128, 2, 3, 200, 333, 1, 1, 0, 0), (FG_FA_TILE128, 1, 0, 0)),
    "tile128_sample_major": ((128, 9, 2, 100, 77, 1, 1, 0, 0), (FG_FA_TILE128, 1, 0, 1)),
    "wide_1037": ((128, 1, 2, 300, 1037, 1, 1, 0, 0), (FG_FA_WIDE_CUT, 2, 17, 0)),
    "wide_cut_middle": ((128, 1, 100, 64, 1100, 1, 1, 0, 0), (FG_FA_WIDE_CUT, 2, 18, 0)),
    "wide_cut_one_tile": ((128, 1, 208, 64, 1024, 1, 1, 0, 0), (FG_FA_WIDE_CUT, 2, 31, 0)),
    "wide_cut_clamped": ((128, 1, 209, 64, 1024, 1, 1, 0, 0), (FG_FA_WIDE_CUT, 2, 31, 0)),
    "wide_no_cut_210": ((128, 1, 210, 64, 1024, 1, 1, 0, 0), (FG_FA_WIDE, 1, 0, 0)),
    "tile72_1000": ((72, 2, 4, 300, 1000, 1, 1, 0, 0), (FG_FA_TILE72, 4, 0, 0)),
    "tile72_sample_major": ((72, 9, 2, 100, 300, 1, 1, 0, 0), (FG_FA_TILE72, 1, 0, 1)),
}


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_shapes_keep_their_kernels(name):
    """A change of the heuristics cannot silently move the engines' shapes, or the GPU tests', to another kernel."""
    (hd, B, H, Lq, Lkv, ldk_mult, scratch, fs, path), want = NAMED[name]
    p = plan(hd, B, H, Lq, Lkv, ldk_mult * H * hd, scratch, fs, path)
    assert p.refusal == 0
    assert (p.kernel, p.nsplit, p.t_cut, p.sample_major) == want
