"""The three kernels `fg_dit_jvp` adds (fastgen_amd/csrc/dit_jvp.hip), each on its own through its `fg_op_dit_*_jvp` entry point against
the fp64 mirror tests/dit_jvp_ref.py (pinned on the CPU by tests/test_dit_jvp_ref.py), on the values the kernel reads (fp32 inputs, or
hi + lo of the bf16 planes), per token row (LayerNorm-modulate, GELU) and per (sample, head) (attention).

Bounds: (relative L2, max |err| / max |ref|) per granule, twice the worst value measured on an MI355X over the cases of this file:
    ln_modulate  y 3.51e-6 / 7.48e-6,  yd 3.07e-6 / 7.45e-6
    attention    out 6.90e-6 / 1.13e-5, outd 9.48e-6 / 2.34e-5
    gelu         a 2.83e-6 / 5.15e-6,  ad 2.89e-6 / 6.27e-6
(every test prints its own figures).  The outputs of ln_modulate and gelu are [hi | lo] bf16 planes, which carry a value to 2^-17 =
7.6e-6 relative: that, not the arithmetic in front of it, is what their figures show.  Discrimination, from the mirror alone: a tangent
without the softmax-derivative term (attention), without the n sd + bd terms (ln_modulate), and the neighbouring sample's tangent
miss these bounds by more than 5 times in every granule (the tests assert it and print by how much)."""
import ctypes

import pytest
import torch

import dit_attention_ref as A
import dit_jvp_ref as J
from fastgen_amd import _lib

pytestmark = pytest.mark.gpu

# (relative L2, max |err| / max |ref|) per granule: 2 x the worst measured (module docstring)
TOL = {
    "ln_y": (7.1e-6, 1.5e-5), "ln_yd": (6.2e-6, 1.5e-5),
    "att_o": (1.4e-5, 2.3e-5), "att_od": (1.9e-5, 4.7e-5),
    "gelu_a": (5.7e-6, 1.1e-5), "gelu_ad": (5.8e-6, 1.3e-5),
}
F64 = torch.float64


def _dev():
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _planes(buf, n):
    """[rows][2 n] bf16 planes -> fp64 hi + lo."""
    b = buf.cpu().double()
    return b[:, :n] + b[:, n:]


def _err(got, ref, dims):
    """(relative L2, max |err| / max |ref|) per granule: the norms run over `dims`."""
    e = got - ref
    return ((e.pow(2).sum(dims).sqrt() / ref.pow(2).sum(dims).sqrt()).max().item(),
            (e.abs().amax(dims) / ref.abs().amax(dims)).max().item())


def _far(mutant, ref, dims, bound):
    """How many times the closest granule of a mutated reference misses the bound (the smaller of the two measures)."""
    e = mutant - ref
    l2 = (e.pow(2).sum(dims).sqrt() / ref.pow(2).sum(dims).sqrt()).min().item() / bound[0]
    mx = (e.abs().amax(dims) / ref.abs().amax(dims)).min().item() / bound[1]
    return min(l2, mx)


def _report(name, figs):
    print(f"\n[dit-jvp-op] {name}: " + "  ".join(f"{k} {v[0]:.2e} / {v[1]:.2e}" for k, v in figs.items()))
    bad = {k: v for k, v in figs.items() if not (v[0] <= TOL[k][0] and v[1] <= TOL[k][1])}
    assert not bad, bad


@pytest.mark.parametrize("D,stride,so,co", [(384, 6 * 384, 0, 384), (1152, 6 * 1152 + 8, 3 * 1152 + 2, 4 * 1152 + 6), (1152, 2 * 1152, 1152, 0)],
                         ids=["D384", "D1152-offsets", "D1152-swapped"])
def test_ln_modulate_jvp(D, stride, so, co):
    """2 images x 256 tokens with their own modulation rows; nonzero scale / shift tangents; rows with a large mean and a small spread."""
    g = torch.Generator().manual_seed(D + so)
    ntok, tpi = 512, 256
    x = torch.randn(ntok, D, generator=g) * (0.2 + 3 * torch.rand(ntok, 1, generator=g)) + 2 * torch.randn(ntok, 1, generator=g)
    xd = torch.randn(ntok, D, generator=g) * 1.5 + 0.5
    mod, modd = torch.randn(2, stride, generator=g), torch.randn(2, stride, generator=g) * 2
    dev = _dev()
    y = torch.full((ntok, 2 * D), float("nan"), dtype=torch.bfloat16, device=dev)
    yd = torch.full_like(y, float("nan"))
    xg, xdg, mg, mdg = (a.to(dev) for a in (x, xd, mod, modd))
    _lib.check(_lib.lib().fg_op_dit_ln_modulate_jvp(_p(xg), _p(xdg), _p(mg), _p(mdg), stride, so, co, _p(y), _p(yd), ntok, D, tpi, _stream()))
    torch.cuda.synchronize()
    sl = lambda m, o: m.double()[:, o:o + D]  # noqa: E731
    args = (x.double().view(2, tpi, D), xd.double().view(2, tpi, D), sl(mod, so), sl(modd, so), sl(mod, co), sl(modd, co))
    ry, ryd = (a.reshape(ntok, D) for a in J.ln_modulate_jvp(*args))
    gy, gyd = _planes(y, D), _planes(yd, D)
    assert bool(torch.isfinite(gy).all() and torch.isfinite(gyd).all())
    # discrimination (from the mirror alone): no n sd + bd terms; the other image's tangent
    cut = J.ln_modulate_jvp(*args, drop_mod_tangent=True)[1].reshape(ntok, D)
    far = _far(cut, ryd, (1,), TOL["ln_yd"]), _far(ryd.roll(tpi, 0), ryd, (1,), TOL["ln_yd"])
    print(f"\n[dit-jvp-op] ln_modulate D {D} mutants miss the bound {far[0]:.3g} x (no n sd + bd), {far[1]:.3g} x (other image)")
    assert min(far) >= 5, far
    _report(f"ln_modulate D {D} stride {stride} offsets {so}/{co}", {"ln_y": _err(gy, ry, (1,)), "ln_yd": _err(gyd, ryd, (1,))})


_ATT = {}


def _attention(H, hd, kind):
    """(got out, got outd, ref out, ref outd, operands as seen) of one case, [B, H, T, hd] fp64; computed once."""
    key = (H, hd, kind)
    if key not in _ATT:
        B, T = 2, 256
        g = torch.Generator().manual_seed(100 * hd + H)
        q, k, v, qd, kd, vd = (torch.randn(B, T, H * hd, generator=g) * s for s in (1.5, 1.5, 1.0, 2.0, 2.0, 3.0))
        qd, kd = qd + 0.7, kd + 1.1  # a part common to every token: the shift tangent of the modulation reaches the keys this way
        if kind == "qk0":
            qd, kd = torch.zeros_like(qd), torch.zeros_like(kd)
        if kind == "v0":
            vd = torch.zeros_like(vd)
        dev = _dev()
        n = B * H * T * hd
        bufs = []
        for a, b, c in ((q, k, v), (qd, kd, vd)):
            qp, kp, vp, lo_off = A.pack("bf16x3", a, b, c, H, hd)
            for pl in (qp, kp, vp):  # the slack behind each plane is never part of a result: poison it
                pl[n:lo_off] = float("nan")
                pl[lo_off + n:] = float("nan")
            bufs += [qp.to(dev), kp.to(dev), vp.to(dev)]
        out = torch.full((B, T, H * hd), float("nan"), device=dev)
        outd = torch.full_like(out, float("nan"))
        _lib.check(_lib.lib().fg_op_dit_attention_jvp(*[_p(b) for b in bufs], _p(out), _p(outd), B, H, hd, T, lo_off, _stream()))
        torch.cuda.synchronize()
        seen = [A.heads_first(A.as_seen("bf16x3", a), H, hd) for a in (q, k, v, qd, kd, vd)]
        ro, rod = J.attention_core_jvp(*seen)
        hf = lambda a: A.heads_first(a.cpu().double(), H, hd)  # noqa: E731
        _ATT[key] = (hf(out), hf(outd), ro, rod, seen)
    return _ATT[key]


@pytest.mark.parametrize("kind", ["full", "qk0", "v0"])
@pytest.mark.parametrize("H,hd", [(3, 64), (2, 72)])
def test_attention_jvp(H, hd, kind):
    """Every (sample, head) with its own data; qk0: qd = kd = 0 (only P vd survives); v0: vd = 0 (only the softmax-derivative term)."""
    go, god, ro, rod, seen = _attention(H, hd, kind)
    assert bool(torch.isfinite(go).all() and torch.isfinite(god).all())
    if kind == "full":  # discrimination: Od = P vd only; the other sample's tangent
        cut = J.attention_core_jvp(*seen, drop_softmax_term=True)[1]
        far = _far(cut, rod, (2, 3), TOL["att_od"]), _far(rod.roll(1, 0), rod, (2, 3), TOL["att_od"])
        print(f"\n[dit-jvp-op] attention H {H} hd {hd} mutants miss the bound {far[0]:.3g} x (Od = P vd only), {far[1]:.3g} x (other sample)")
        assert min(far) >= 5, far
    _report(f"attention H {H} hd {hd} {kind}", {"att_o": _err(go, ro, (2, 3)), "att_od": _err(god, rod, (2, 3))})


def test_attention_jvp_primal_does_not_depend_on_the_tangent():
    for H, hd in ((3, 64), (2, 72)):
        assert torch.equal(_attention(H, hd, "full")[0], _attention(H, hd, "qk0")[0])
        assert torch.equal(_attention(H, hd, "full")[0], _attention(H, hd, "v0")[0])


def test_gelu_jvp():
    M, K = 512, 1536
    g = torch.Generator().manual_seed(9)
    h = torch.rand(M, K, generator=g) * 12 - 6
    h[0, :1001] = torch.linspace(-6, 6, 1001)
    hd = torch.randn(M, K, generator=g) * 2
    dev = _dev()
    a = torch.full((M, 2 * K), float("nan"), dtype=torch.bfloat16, device=dev)
    ad = torch.full_like(a, float("nan"))
    hg, hdg = h.to(dev), hd.to(dev)
    _lib.check(_lib.lib().fg_op_dit_gelu_jvp(_p(hg), _p(hdg), _p(a), _p(ad), M, K, _stream()))
    torch.cuda.synchronize()
    ra, rad = J.gelu_jvp(h.double(), hd.double())
    ga, gad = _planes(a, K), _planes(ad, K)
    assert bool(torch.isfinite(ga).all() and torch.isfinite(gad).all())
    _report("gelu 512 x 1536", {"gelu_a": _err(ga, ra, (1,)), "gelu_ad": _err(gad, rad, (1,))})
