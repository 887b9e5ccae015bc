"""`ConditionSlot` alone: a condition is the same thing again only as the same tensor OBJECT at the same in-place version and shape
(with the same plain extras); anything else is handed to the handle again."""
import torch

from fastgen_amd.networks.Wan._shared import ConditionSlot


def _slot(*tensors, extra=()):
    s = ConditionSlot()
    assert not s.same(*tensors, extra=extra)  # (nothing remembered yet)
    s.remember(*tensors, extra=extra)
    return s


def test_same_object_same_version_hits():
    t = torch.randn(2, 3)
    s = _slot(t)
    assert s.same(t) and s.same(t)


def test_version_bump_misses():
    t = torch.randn(2, 3)
    s = _slot(t)
    t.mul_(1.0)
    assert not s.same(t)
    s.remember(t)
    assert s.same(t)


def test_new_object_on_the_same_storage_misses():
    t = torch.randn(2, 3)
    s = _slot(t)
    assert not s.same(t.detach())
    assert not s.same(t.view_as(t))


def test_equal_valued_clone_misses():
    t = torch.randn(2, 3)
    assert not _slot(t).same(t.clone())


def test_inference_tensor_hits_without_reading_its_version():
    with torch.inference_mode():
        t = torch.randn(2, 3)
    assert t.is_inference()
    s = _slot(t)  # (`t._version` would raise)
    assert s.same(t)
    with torch.inference_mode():
        assert s.same(t) and not s.same(torch.randn(2, 3))


def test_deleted_tensor_then_a_new_one_of_the_same_shape_misses():
    t = torch.randn(2, 3)
    s = _slot(t)
    del t
    assert not s.same(torch.randn(2, 3))
    assert not s.same(None)


def test_pair_with_none_hits_only_the_same_pair():
    t, u = torch.randn(2, 3), torch.randn(2, 3)
    s = _slot(t, None)
    assert s.same(t, None)
    assert not s.same(t, u) and not s.same(u, None) and not s.same(None, t) and not s.same(None, None) and not s.same(t)
    s.remember(t, u)
    assert s.same(t, u) and not s.same(t, None) and not s.same(u, t)


def test_changed_extra_misses():
    t = torch.randn(2, 3)
    s = _slot(t, extra=(5,))
    assert s.same(t, extra=(5,)) and not s.same(t, extra=(6,)) and not s.same(t)
    scales = _slot(extra=[1.0, 0.5])
    assert scales.same(extra=[1.0, 0.5]) and not scales.same(extra=[1.0, 0.25]) and not scales.same(extra=[1.0])


def test_forget_misses():
    t = torch.randn(2, 3)
    s = _slot(t, extra=(5,))
    s.forget()
    assert not s.same(t, extra=(5,))
