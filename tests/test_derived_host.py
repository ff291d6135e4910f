"""mixdq_amd/derived.py on plain CPU tensors: the staleness key (identity + version + extra), the in-place rewrite at
equal metadata, the fresh start at other metadata, refresh / drop, and the shared module lifecycle."""
import torch
import torch.nn as nn

from mixdq_amd import derived as D


class Counting:
    """build(old, *sources) -> (2 * s0, s1 + 1, ...), counting its calls and keeping what `old` it was given."""

    def __init__(self):
        self.calls, self.olds = 0, []

    def __call__(self, old, *sources):
        self.calls += 1
        self.olds.append(old)
        return tuple(s * 2 if i == 0 else s + 1 for i, s in enumerate(sources))


def _ptrs(outs):
    return [t.data_ptr() for t in outs]


def test_a_hit_calls_nothing_and_returns_the_same_objects():
    h, b = {}, Counting()
    a, c = torch.arange(6.0).reshape(2, 3), torch.ones(4)
    first = D.derive(h, "k", (a, c), b)
    assert b.calls == 1 and b.olds == [None]
    assert torch.equal(first[0], a * 2) and torch.equal(first[1], c + 1)
    for _ in range(3):
        again = D.derive(h, "k", (a, c), b)
        assert again is first and all(x is y for x, y in zip(again, first))
    assert b.calls == 1 and D.stored(h, "k") is first and D.stored(h, "other") is None and D.stored(None, "k") is None


def test_an_in_place_write_rebuilds_once_at_the_same_addresses():
    h, b = {}, Counting()
    a, c = torch.arange(6.0).reshape(2, 3), torch.ones(4)
    first = D.derive(h, "k", (a, c), b)
    ptrs = _ptrs(first)
    a.mul_(2)
    got = D.derive(h, "k", (a, c), b)
    assert b.calls == 2 and b.olds[1] is first                     # (the builder is offered the stored tensors)
    assert got is first and _ptrs(got) == ptrs and torch.equal(got[0], a * 2) and torch.equal(got[0][1], a[1] * 2)
    assert D.derive(h, "k", (a, c), b) is first and b.calls == 2   # re-keyed: a hit again


def test_a_replaced_source_of_equal_metadata_rebuilds_once_at_the_same_addresses():
    h, b = {}, Counting()
    a, c = torch.arange(6.0).reshape(2, 3), torch.ones(4)
    first = D.derive(h, "k", (a, c), b)
    ptrs = _ptrs(first)
    a2 = torch.full((2, 3), 5.0)
    got = D.derive(h, "k", (a2, c), b)
    assert b.calls == 2 and got is first and _ptrs(got) == ptrs and torch.equal(got[0], a2 * 2)
    assert D.derive(h, "k", (a2, c), b) is first and b.calls == 2
    assert D.derive(h, "k", (a2,), b) is not first and b.calls == 3           # another number of sources: no hit


def test_a_source_of_another_dtype_or_shape_yields_new_tensors():
    for other in (torch.arange(6.0, dtype=torch.float64).reshape(2, 3), torch.arange(8.0).reshape(2, 4)):
        h, b = {}, Counting()
        a, c = torch.arange(6.0).reshape(2, 3), torch.ones(4)
        first = D.derive(h, "k", (a, c), b)
        first0 = first[0].clone()
        got = D.derive(h, "k", (other, c), b)
        assert b.calls == 2 and got is not first and got[0].data_ptr() != first[0].data_ptr()
        assert (got[0].dtype, got[0].shape) == (other.dtype, other.shape) and torch.equal(got[0], other * 2)
        assert torch.equal(first[0], first0)                       # nothing was written into the old tensors
        assert D.derive(h, "k", (other, c), b) is got and b.calls == 2


def test_an_output_that_is_a_source_is_not_copied_onto_itself():
    copies = []

    class Spy(torch.Tensor):                                       # counts copy_ calls per destination
        @classmethod
        def __torch_function__(cls, func, types, args=(), kwargs=None):
            if func is torch.Tensor.copy_:
                copies.append(args[0].data_ptr())
            return super().__torch_function__(func, types, args, kwargs or {})

    w, bias = torch.arange(4.0), torch.ones(4).as_subclass(Spy)

    def build(old, w, bias):
        return (w * 3).as_subclass(Spy), bias.detach()             # (the derived bias IS the parameter's storage)

    h = {}
    first = D.derive(h, "k", (w, bias), build)
    assert first[1].data_ptr() == bias.data_ptr() and copies == []
    w.add_(1)
    bias.add_(1)
    copies.clear()
    got = D.derive(h, "k", (w, bias), build)
    assert got is first and torch.equal(got[0], w * 3) and torch.equal(got[1], torch.full((4,), 2.0))
    assert copies == [first[0].data_ptr()]                         # the weight was copied, the bias was not


def test_a_builder_that_writes_into_the_stored_tensors_is_not_copied_either():
    def build(old, s):
        if old is None:
            return (s.clone(),)
        old[0].copy_(s)
        return old

    h, s = {}, torch.arange(3.0)
    first = D.derive(h, "k", (s,), build)
    s.mul_(4)
    assert D.derive(h, "k", (s,), build) is first and torch.equal(first[0], s)
    # `into`: a first build lands in storage the caller keeps (a row of a kept buffer)
    buf = torch.zeros(2, 3)
    row = D.derive({}, "row", (s,), build, into=(buf[:1],))
    assert row[0].data_ptr() == buf.data_ptr() and torch.equal(buf[0], s) and not buf[1].any()


def test_refresh_rebuilds_only_the_stale_records():
    h, b1, b2 = {}, Counting(), Counting()
    s1, s2 = torch.ones(3), torch.ones(3)
    o1, o2 = D.derive(h, 1, (s1,), b1), D.derive(h, 2, (s2,), b2)
    D.refresh(h)
    assert (b1.calls, b2.calls) == (1, 1)
    s2.add_(1)
    D.refresh(h)
    assert (b1.calls, b2.calls) == (1, 2) and D.stored(h, 2) is o2 and torch.equal(o2[0], s2 * 2)
    D.refresh(h)                                                   # a second visit (a parent's hook after a child's): hits
    assert (b1.calls, b2.calls) == (1, 2) and D.stored(h, 1) is o1
    D.refresh(None)
    D.refresh({})


def test_drop_empties_the_holder():
    h, b = {}, Counting()
    s = torch.ones(3)
    first = D.derive(h, "k", (s,), b)
    D.drop(h)
    assert h == {} and D.stored(h, "k") is None
    assert D.derive(h, "k", (s,), b) is not first and b.calls == 2
    D.drop(None)


def test_extra_takes_part_in_the_key():
    h, b = {}, Counting()
    s = torch.ones(3)
    first = D.derive(h, "k", (s,), b, extra=(4, "a"))
    assert D.derive(h, "k", (s,), b, extra=(4, "a")) is first and b.calls == 1
    assert D.derive(h, "k", (s,), b, extra=(5, "a")) is first and b.calls == 2     # same metadata: rebuilt in place
    assert D.derive(h, "k", (s,), b, extra=(5, "a")) is first and b.calls == 2
    assert D.fresh(h["k"], (s,), (5, "a")) and not D.fresh(h["k"], (s,), (4, "a")) and not D.fresh(None, (s,))
    D.refresh(h)                                                   # a refresh keeps the record's own extra
    assert b.calls == 2


class _Child(D.DerivedWeights, nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(3, 2)
        self.builds = Counting()
        self.dropped = 0
        self._init_derived()

    def _derive(self):
        return dict(w=((self.lin.weight, self.lin.bias), self.builds))

    def _drop_derived(self):
        super()._drop_derived()
        self.dropped += 1


class _Parent(nn.Module):
    """As SDXLUNet: its own load hook walks the children again after theirs have run."""

    def __init__(self):
        super().__init__()
        self.child = _Child()
        self.register_load_state_dict_post_hook(D.after_load)

    def refresh_derived_(self):
        for m in self.modules():
            if m is not self and hasattr(m, "refresh_derived_"):
                m.refresh_derived_()


def test_module_lifecycle_a_load_rewrites_in_place_once_a_move_drops():
    p, q = _Parent(), _Parent()
    c = p.child
    w2, b1 = c._derived()["w"]
    ptrs = (w2.data_ptr(), b1.data_ptr())
    assert c.builds.calls == 1 and c._derived()["w"][0] is w2 and c.builds.calls == 1
    p.load_state_dict(q.state_dict())                              # the child's hook, then the parent's walk: ONE build
    assert c.builds.calls == 2 and c.dropped == 0
    got = c._derived()["w"]
    assert c.builds.calls == 2 and (got[0].data_ptr(), got[1].data_ptr()) == ptrs
    assert torch.equal(got[0], q.child.lin.weight * 2) and torch.equal(got[1], q.child.lin.bias + 1)
    p.load_state_dict(_Parent().state_dict())                      # a second load is seen too
    assert c.builds.calls == 3 and not torch.equal(c._derived()["w"][0], q.child.lin.weight * 2)
    # assign=True with another dtype: the derived tensors start over, with whatever else goes with them
    p.load_state_dict({k: v.double() for k, v in q.state_dict().items()}, assign=True)
    assert not D.holder_of(c) and c.dropped == 1 and c._derived()["w"][0].dtype == torch.float64
    p.float()                                                      # a move or a dtype change drops them
    assert not D.holder_of(c) and c.dropped == 2
    r = _Parent()
    r.load_state_dict(q.state_dict())                              # a load before anything was derived builds nothing
    assert r.child.builds.calls == 0 and not D.holder_of(r.child)
