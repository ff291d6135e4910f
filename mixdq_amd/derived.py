"""Tensors computed from weights, cached, and read by captured graphs through raw addresses: the one mechanism
(DESIGN.md "Derived tensors").  A holder is a plain dict of records

    key -> (sources, versions, outs, extra, build)

`sources` are the tensors the outputs were computed from, `versions` their in-place `_version` at that time, `outs`
the tuple of derived tensors, `extra` whatever else the result depends on and `build(old, *sources)` the function that
computes them (`old`: the stored outs or None; a builder may write into them and return them).
"""
import torch


def fresh(rec, sources, extra=()) -> bool:
    """The record was made from these very tensors, at their current versions, with this `extra`.  Host-only."""
    return (rec is not None and len(rec[0]) == len(sources) and all(a is b for a, b in zip(rec[0], sources))
            and rec[1] == tuple(t._version for t in sources) and rec[3] == extra)


def record(sources, extra, outs, build=None):
    return (tuple(sources), tuple(t._version for t in sources), outs, extra, build)


def _meta(t):
    return (t.shape, t.dtype, t.device)


def derive(holder: dict, key, sources, build, extra=(), into=None):
    """The derived tensors of `key`.  A hit returns the stored ones and touches nothing on the device.  A stale record
    is rebuilt: where every new tensor has the stored one's (shape, dtype, device) the stored tensors are rewritten
    in place and returned -- their addresses never change -- otherwise (or with no record) what `build` returned is
    stored.  `into`: tensors the caller keeps (a row of a kept buffer) that stand in for the stored ones of a first
    build, so the result lives there from the start."""
    rec = holder.get(key)
    if fresh(rec, sources, extra):
        return rec[2]
    old = rec[2] if rec is not None else into
    with torch.no_grad():
        new = tuple(build(old, *sources))
        if old is not None and len(old) == len(new) and all(_meta(o) == _meta(n) for o, n in zip(old, new)):
            for o, n in zip(old, new):
                if o.data_ptr() != n.data_ptr():       # (a derived bias may BE the parameter; a builder may have
                    o.copy_(n)                         #  written into the stored tensor itself)
            new = old
    holder[key] = record(sources, extra, new, build)
    return new


def stored(holder, key):
    """The stored tensors of `key` as they are, without a staleness test (inside a captured step), or None."""
    rec = (holder or {}).get(key)
    return None if rec is None else rec[2]


def refresh(holder) -> None:
    """Run the staleness test of every record now, against the sources it was made from: after they were written in
    place (load_state_dict, shard.broadcast_module_state) the derived tensors follow, at their addresses.  A source
    that was REPLACED is seen by its owner's next derive() call."""
    for key, (sources, _, _, extra, build) in list((holder or {}).items()):
        derive(holder, key, sources, build, extra)


def drop(holder) -> None:
    """Forget everything: after a move or a dtype change every tensor has a new address anyway."""
    if holder is not None:
        holder.clear()


def holder_of(mod) -> dict:
    return mod.__dict__.setdefault("_derived_tensors", {})


def after_load(mod, _incompatible_keys):
    mod.refresh_derived_()


class DerivedWeights:
    """Lifecycle of an nn.Module that declares `_derive() -> {name: (sources, build)}`: `_derived()` is the dict of
    derived tuples; a load rewrites them in place (or, where load_state_dict(assign=True) changed their metadata,
    starts over); a move drops them.  `_drop_derived()` is the hook for whatever else goes with them."""

    def _init_derived(self):
        self.register_load_state_dict_post_hook(after_load)

    def _derived(self):
        h = holder_of(self)
        return {k: derive(h, k, s, b) for k, (s, b) in self._derive().items()}

    def _drop_derived(self):
        drop(holder_of(self))

    def refresh_derived_(self):
        before = {k: r[2] for k, r in holder_of(self).items()}
        if before and any(self._derived().get(k) is not v for k, v in before.items()):
            self._drop_derived()
        return self

    def _apply(self, fn, recurse=True):          # .to() / .cuda() / .half(): the weights move, the derived ones go
        self._drop_derived()
        return super()._apply(fn, recurse)
