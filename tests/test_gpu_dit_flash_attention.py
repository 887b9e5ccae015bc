"""fg_op_dit_attention (fastgen_amd/csrc/dit.hip: dit_attention_kernel at 256 tokens, dit_flash_kernel at every multiple of 256) per
element against fp64 over the full tensor, bounds and inputs of tests/dit_attention_ref.py (whose teeth tests/test_dit_attention_ref.py
shows on the CPU).  B 2, 3 heads, head dim 64 and 72, bf16 and split-bf16, 256 / 512 / 768 / 1024 tokens (one block pair = one rescale;
a block count that is no power of two; the engine's 1024)."""
import ctypes

import pytest
import torch

import dit_attention_ref as A
from fastgen_amd import _lib

pytestmark = pytest.mark.gpu

B, H = 2, 3
FG_EINVAL = 1
MODES = {"bf16": _lib.FG_DTYPE_BF16, "bf16x3": _lib.FG_DTYPE_BF16X3}
INPUTS = ("gaussian", "late", "early", "equal", "selection")
_CACHE = {}


def _case(kind, mode, hd, T):
    """(q, k, v as the mode sees them, reference, extra) - computed once per case and shared (nothing changes them)."""
    key = (kind, mode, hd, T)
    if key not in _CACHE:
        extra = None
        if kind == "gaussian":
            q, k, v = A.gaussian(B, H, hd, T)
        elif kind in ("late", "early"):
            q, k, v, extra = A.spiked(kind, B, H, hd, T)
        elif kind == "equal":
            q, k, v = A.all_equal(B, H, hd, T)
        else:
            q, k, v, extra = A.block_selection(B, H, hd, T)
        qs, ks, vs = (A.as_seen(mode, x) for x in (q, k, v))
        _CACHE[key] = (q, k, v, A.reference(qs, ks, vs, H, hd), float(vs.abs().max()), extra)
    return _CACHE[key]


def _op(mode, q, k, v, hd, path, expect=0, fill=None):
    """One call of the op on logical [b, T, H hd] operands; the output as fp64 [b, T, H hd] on the CPU (and the return code)."""
    dev = torch.device("cuda:0")
    b, T = q.shape[:2]
    qp, kp, vp, lo_off = (x.to(dev) if torch.is_tensor(x) else x for x in A.pack(mode, q, k, v, H, hd))
    out = torch.empty(b, T, H * hd, dtype=torch.bfloat16 if mode == "bf16" else torch.float32, device=dev)
    if fill is not None:
        out.fill_(fill)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = _lib.lib().fg_op_dit_attention(MODES[mode], p(qp), p(kp), p(vp), p(out), b, H, hd, T, lo_off, path,
                                        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.lib().fg_last_error().decode())
    return out.cpu()


def _worst(got, ref, bnd):
    return float(((got.double() - ref["want"]).abs() / bnd).max())


@pytest.mark.parametrize("T", [256, 512, 768, 1024])
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("hd", [64, 72])
def test_every_element_within_the_bound(hd, mode, T):
    paths = (0, 1, 2) if T == 256 else (0, 2)
    report, bad = [], []
    for kind in INPUTS:
        q, k, v, ref, vmax, extra = _case(kind, mode, hd, T)
        if kind in ("late", "early"):  # the leading key of every chosen row lies in the block the input names
            s = A.as_seen(mode, q).view(B, T, H, hd).transpose(1, 2) @ A.as_seen(mode, k).view(B, T, H, hd).transpose(1, 2).transpose(2, 3)
            for b, h, qi, kj in extra:
                top = float(s[b, h, qi, kj]) * 1.4426950408889634 / hd ** 0.5
                assert abs(top - float(ref["top"][b, qi, h])) <= 1e-9 * abs(top) and float(ref["lead"][b, qi, h]) > 8
                assert kj >= T - A.KB if kind == "late" else kj < A.KB
        outs = {}
        for path in paths:
            flash = path == 2 or (path == 0 and T != 256)
            got = outs[path] = _op(mode, q, k, v, hd, path)
            w = _worst(got, ref, A.bound(mode, ref, hd, T, vmax, A.kblocks(T, flash)))
            report.append(f"{kind}/p{path} {w:.2f}")
            if not (bool(torch.isfinite(got).all()) and w <= 1.0):
                bad.append((kind, path, w))
        if kind == "selection" and mode == "bf16":  # a lead of more than 40 bits: the chosen key's value row, bit for bit
            want = torch.gather(A.as_seen(mode, v).view(B, T, H, hd).transpose(1, 2), 2, extra[..., None].expand(B, H, T, hd))
            for path in paths:
                if not torch.equal(outs[path].double().view(B, T, H, hd).transpose(1, 2), want):
                    bad.append((kind, path, "not the selected row"))
        if kind == "equal":  # uniform weights: the mean of v
            mean = A.as_seen(mode, v).mean(1, keepdim=True)
            assert float((ref["want"] - mean).abs().max()) < 1e-12
        if T == 256:
            if not torch.equal(outs[0], outs[1]):  # the engine's kernel at 256 tokens is the whole-sequence one, unchanged
                bad.append((kind, "path 0 != path 1"))
            both = A.bound(mode, ref, hd, T, vmax, 1) + A.bound(mode, ref, hd, T, vmax, T // A.KB)
            if not bool(((outs[2].double() - outs[1].double()).abs() <= both).all()):
                bad.append((kind, "path 2 against path 1"))
    print(f"\n[dit-flash] hd {hd} {mode} T {T}: worst |err| / bound  " + "  ".join(report))
    assert not bad, bad


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("hd", [64, 72])
def test_batch_independence(hd, mode):
    for T in (256, 512):
        q, k, v = _case("late", mode, hd, T)[:3]
        both = _op(mode, q, k, v, hd, 0)
        for b in range(B):
            assert torch.equal(both[b:b + 1], _op(mode, q[b:b + 1], k[b:b + 1], v[b:b + 1], hd, 0))


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_refusals_leave_out_untouched(mode):
    hd = 64
    for T, path in ((300, 0), (300, 2), (512, 1), (128, 0), (256, 3)):
        g = torch.Generator().manual_seed(T)
        q, k, v = (torch.randn(1, T, H * hd, generator=g) for _ in range(3))
        out = _op(mode, q, k, v, hd, path, expect=FG_EINVAL, fill=-7.0)
        assert bool((out == -7.0).all())
    assert "path" in _lib.lib().fg_last_error().decode()
