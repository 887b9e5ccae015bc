"""The bounds of tests/dit_attention_ref.py have teeth (CPU): an fp64 model of the flash form agrees with the reference, models with the
mode's own roundings stay inside the mode's bound, and models with one defect each - no rescale at a change of maximum, the row sum
rescaled but not O, P rounded to bf16 in the split mode - are rejected on the inputs of tests/test_gpu_dit_flash_attention.py."""
import pytest
import torch

import dit_attention_ref as A

B, H = 1, 3


def _ref(mode, q, k, v, hd):
    qs, ks, vs = (A.as_seen(mode, x) for x in (q, k, v))
    return qs, ks, vs, A.reference(qs, ks, vs, H, hd)


def _excess(got, ref, bnd):
    """max of |got - want| / bound"""
    return float(((got - ref["want"]).abs() / bnd).max())


@pytest.mark.parametrize("hd", [64, 72])
@pytest.mark.parametrize("T", [256, 512, 768])
def test_flash_model_is_the_reference(hd, T):
    q, k, v, _ = A.spiked("late", B, H, hd, T)
    qs, ks, vs, ref = _ref("bf16x3", q, k, v, hd)
    assert float((A.flash_fp64(qs, ks, vs, H, hd) - ref["want"]).abs().max()) < 1e-12
    # the leading key of every chosen query lies in the last block
    q2, k2, v2 = A.gaussian(B, H, hd, T)
    assert float((A.flash_fp64(q2, k2, v2, H, hd) - A.reference(q2, k2, v2, H, hd)["want"]).abs().max()) < 1e-12


@pytest.mark.parametrize("hd", [64, 72])
@pytest.mark.parametrize("mode,rounding", [("bf16", "p_bf16"), ("bf16x3", "p_split")])
def test_bounds_accept_the_modes_own_roundings(hd, mode, rounding):
    T = 512
    for q, k, v in (A.gaussian(B, H, hd, T), A.two_level(B, H, hd, T), A.spiked("early", B, H, hd, T)[:3]):
        qs, ks, vs, ref = _ref(mode, q, k, v, hd)
        got = A.flash_fp64(qs, ks, vs, H, hd, defect=rounding)
        if mode == "bf16":
            got = got.float().bfloat16().double()
        assert _excess(got, ref, A.bound(mode, ref, hd, T, float(vs.abs().max()), T // A.KB)) <= 1.0


@pytest.mark.parametrize("hd", [64, 72])
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("defect", ["no_rescale", "rescale_l"])
@pytest.mark.parametrize("T", [512, 1024])
def test_bounds_reject_a_missing_rescale(hd, mode, defect, T):
    """Late maximum: the blocks before the last were accumulated against a maximum many bits too low."""
    q, k, v, picks = A.spiked("late", B, H, hd, T)
    qs, ks, vs, ref = _ref(mode, q, k, v, hd)
    bnd = A.bound(mode, ref, hd, T, float(vs.abs().max()), T // A.KB)
    bad = A.flash_fp64(qs, ks, vs, H, hd, defect=defect)
    err = ((bad - ref["want"]).abs() / bnd).view(B, T, H, hd).amax(-1)
    for b, h, qi, _ in picks:  # every chosen query row, on its own
        assert float(err[b, qi, h]) > 10.0
    # Gaussian rows move their maximum too: the defect shows without the spike as well
    q, k, v = A.gaussian(B, H, hd, T)
    qs, ks, vs, ref = _ref(mode, q, k, v, hd)
    assert _excess(A.flash_fp64(qs, ks, vs, H, hd, defect=defect), ref, A.bound(mode, ref, hd, T, float(vs.abs().max()), T // A.KB)) > 10.0


@pytest.mark.parametrize("hd", [64, 72])
@pytest.mark.parametrize("T", [256, 1024])
def test_split_bound_rejects_p_rounded_to_bf16(hd, T):
    q, k, v = A.two_level(B, H, hd, T)
    qs, ks, vs, ref = _ref("bf16x3", q, k, v, hd)
    bnd = A.bound("bf16x3", ref, hd, T, float(vs.abs().max()), T // A.KB)
    assert _excess(A.flash_fp64(qs, ks, vs, H, hd, defect="p_bf16"), ref, bnd) > 2.0  # (4.0 at 1024 tokens, 11 at 256)
    assert _excess(A.flash_fp64(qs, ks, vs, H, hd, defect="p_split"), ref, bnd) <= 1.0
    # ... and the bf16 bound, rightly, accepts it
    assert _excess(A.flash_fp64(qs, ks, vs, H, hd, defect="p_bf16"), ref, A.bound("bf16", ref, hd, T, float(vs.abs().max()), T // A.KB)) <= 1.0


@pytest.mark.parametrize("where", ["late", "early"])
def test_spiked_inputs_put_the_leading_key_where_they_say(where):
    hd, T = 64, 768
    q, k, v, picks = A.spiked(where, B, H, hd, T)
    qs, ks, vs, ref = _ref("bf16", q, k, v, hd)
    s = (qs.view(B, T, H, hd).transpose(1, 2) @ ks.view(B, T, H, hd).transpose(1, 2).transpose(2, 3))
    for b, h, qi, kj in picks:
        assert int(s[b, h, qi].argmax()) == kj and (kj >= T - A.KB if where == "late" else kj < A.KB)


def test_pack_layout():
    hd, T = 72, 256
    q, k, v = A.gaussian(2, H, hd, T)
    for mode in ("bf16", "bf16x3"):
        qp, kp, vp, lo_off = A.pack(mode, q, k, v, H, hd)
        n = 2 * H * T * hd
        assert qp.numel() == (n + 32 * T) * (2 if mode == "bf16x3" else 1) and lo_off == (0 if mode == "bf16" else n + 32 * T)
        got = qp[:n].double() + (qp[lo_off:lo_off + n].double() if lo_off else 0)
        assert torch.equal(got.view(2, H, T, hd)[1, 2, 17], A.as_seen(mode, q)[1, 17, 2 * hd:3 * hd])
        gv = vp[:n].double() + (vp[lo_off:lo_off + n].double() if lo_off else 0)
        assert torch.equal(gv.view(2, H, hd, T)[1, 2, :, 17], A.as_seen(mode, v)[1, 17, 2 * hd:3 * hd])
