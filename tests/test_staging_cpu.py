"""CPU: sos_wsod_amd.staging — when a compute-dtype copy of a parameter counts as current, on CPU tensors with `build` callables that
count their calls and fill the buffer (no kernel, no device)."""
import copy
import gc
import importlib.util
import os
import pickle
import sys
import weakref

import torch

# by file path, under a name of its own: the module needs neither the package (whose import loads the HIP library) nor ops
_spec = importlib.util.spec_from_file_location(
    "staging_under_test", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sos-wsod_amd", "staging.py"))
staging = sys.modules[_spec.name] = importlib.util.module_from_spec(_spec)          # (registered: pickle looks classes up by module)
_spec.loader.exec_module(staging)


class _Owner(torch.nn.Module):
    """owns parameters and a StageCache the way the backbone / the heads do"""

    def __init__(self, n=2):
        super().__init__()
        self.ws = torch.nn.ParameterList([torch.nn.Parameter(torch.full((3, 4), float(i + 1))) for i in range(n)])
        self.cache = staging.StageCache()
        self.calls = 0

    def staged(self, name, sources, dtype=torch.bfloat16, shape=None, register=True):
        shape = shape or (sum(p.shape[0] for p in sources), 4)

        def build(bufs):
            self.calls += 1
            bufs[0].copy_(torch.cat([p.detach() for p in sources], 0)[:shape[0]])
        slot, built = self.cache.lookup(name, sources, (shape,), dtype, sources[0].device, build)
        row = 0
        for j, p in enumerate(sources if built and register else ()):
            staging.register(p, 1, dtype, stage0=slot.bufs[0][row:row + p.shape[0]], d0=4, ld0=4, slots=[(slot, j)])
            row += p.shape[0]
        return slot.bufs[0]


def _optimizer_update(params):
    """what HipSGD does around its kernel: one epoch per call, then per parameter "updated" (the kernel writes behind torch's
    version counters and rewrites the registered copies itself)"""
    staging.params_written()
    for p in params:
        versions = p._version
        p.data.add_(1.0)
        ent = staging.entry_of(p)
        if ent is not None:
            ent["stage0"].copy_(p.detach())
        assert p._version == versions
        staging.updated(p)


def test_hit_rebuild_in_place_and_changed_spec():
    m = _Owner()
    w = m.ws[0]
    a = m.staged("a", [w])
    assert m.cache.builds == 1 and m.calls == 1 and m.cache.is_current("a") and torch.equal(a.float(), w.detach())
    assert m.staged("a", [w]) is a and m.cache.builds == 1 and m.calls == 1            # a hit: same tensor object, nothing built
    assert m.cache.buffers("a")[0] is a
    ptr = a.data_ptr()
    with torch.no_grad():
        w.mul_(2.0)                                                                   # torch's version counter moves
    assert not m.cache.is_current("a")
    b = m.staged("a", [w])
    assert m.cache.builds == 2 and b.data_ptr() == ptr and torch.equal(b.float(), w.detach())     # rebuilt into the same memory
    c = m.staged("a", [w], dtype=torch.float32)                                       # another dtype: a new buffer
    assert m.cache.builds == 3 and c.dtype == torch.float32 and c.data_ptr() != ptr
    d = m.staged("a", [w], dtype=torch.float32, shape=(2, 4))                          # another shape: a new buffer
    assert m.cache.builds == 4 and tuple(d.shape) == (2, 4) and d.data_ptr() != c.data_ptr()
    assert not m.cache.is_current("never staged")


def test_optimizer_update_keeps_registered_slots_current_per_parameter():
    m = _Owner()
    w0, w1 = m.ws
    a, b = m.staged("a", [w0]), m.staged("b", [w1])
    _optimizer_update([w0])                                                           # one bucket: w1 is not touched
    assert m.cache.is_current("a") and m.cache.is_current("b")
    assert m.staged("a", [w0]) is a and m.staged("b", [w1]) is b and m.cache.builds == 2 and m.calls == 2
    assert torch.equal(a.float(), w0.detach())
    _optimizer_update([w1])                                                           # the next bucket leaves the first one's stamp alone
    assert m.cache.is_current("a") and m.cache.is_current("b") and m.cache.builds == 2
    # a kernel update nobody re-stamps (an unregistered copy) is a miss
    c = m.staged("c", [w0], register=False)
    _optimizer_update([w0])
    assert m.cache.is_current("a") and not m.cache.is_current("c")
    assert m.staged("c", [w0]) is c and m.cache.builds == 4 and torch.equal(c.float(), w0.detach())


def test_invalidate_all_stales_every_slot_of_every_cache():
    m, n = _Owner(), _Owner()
    m.staged("a", [m.ws[0]]); m.staged("b", [m.ws[1]]); n.staged("a", [n.ws[0]])
    before = staging.epochs()
    staging.invalidate_all()
    after = staging.epochs()
    assert after[0] > before[0] and after[1] == before[1] and after[2] > before[2]
    assert not m.cache.is_current("a") and not m.cache.is_current("b") and not n.cache.is_current("a")
    staging.buffers_written()
    assert staging.epochs()[1] == after[1] + 1


def test_two_source_slot_is_stamped_per_source():
    """the packed predictor operand: one buffer, one registry entry per source (a row slice each)"""
    m = _Owner()
    w0, w1 = m.ws
    packed = m.staged("heads", [w0, w1])
    assert tuple(packed.shape) == (6, 4)
    assert staging.entry_of(w0)["stage0"].data_ptr() == packed.data_ptr()
    assert staging.entry_of(w1)["stage0"].data_ptr() == packed[3:].data_ptr()
    staging.params_written()
    w1.data.add_(1.0)
    staging.mark_updated(w1)                                                          # written, not stamped: stale through source 1 only
    assert not m.cache.is_current("heads")
    slot = m.cache.get("heads")
    assert slot.keys[0] == staging.param_key(w0) and slot.keys[1] != staging.param_key(w1)
    slot.stamp(1, staging.param_key(w1))
    assert m.cache.is_current("heads")
    _optimizer_update([w0, w1])
    assert m.cache.is_current("heads") and m.cache.builds == 1 and torch.equal(packed.float(), torch.cat([w0.detach(), w1.detach()]))


def test_second_mode_joins_the_one_registry_entry():
    """a conv weight staged in mode 0 and later in mode 1, registered the way VGG16.staged_weight does — from the slots that
    exist, again after each build: ONE kind-2 entry that ends up with both buffers, and the update re-stamps both slots"""
    m = _Owner(1)
    w = m.ws[0]

    def stage(mode):
        slot, built = m.cache.lookup((id(w), mode), (w,), ((3, 4),), torch.bfloat16, w.device, lambda bufs: bufs[0].copy_(w.detach()))
        assert built
        s0, s1 = m.cache.get((id(w), 0)), m.cache.get((id(w), 1))
        staging.register(w, 2, torch.bfloat16, stage0=None if s0 is None else s0.bufs[0], stage1=None if s1 is None else s1.bufs[0],
                         slots=[(s, 0) for s in (s0, s1) if s is not None])
        return slot.bufs[0]
    b0 = stage(0)
    n = len(staging.REGISTRY)
    ent = staging.entry_of(w)
    assert ent["kind"] == 2 and ent["stage0"] is b0 and ent["stage1"] is None
    b1 = stage(1)
    ent = staging.entry_of(w)
    assert len(staging.REGISTRY) == n and ent["stage0"] is b0 and ent["stage1"] is b1 and len(ent["slots"]) == 2
    _optimizer_update([w])
    assert m.cache.is_current((id(w), 0)) and m.cache.is_current((id(w), 1)) and m.cache.builds == 2
    del m, w, ent
    gc.collect()
    assert len(staging.REGISTRY) == n - 1


def test_staging_registry_does_not_keep_parameters_alive():
    """staging.register holds the parameter weakly and drops the entry (with the staged copies) when the parameter dies; an id
    that a live parameter has taken over keeps its entry.  (A strong reference leaked every deleted model's fc6 weight and its copies.)"""
    w = torch.nn.Parameter(torch.zeros(4, 4))
    staged = torch.zeros(4, 4, dtype=torch.bfloat16)
    staging.register(w, 1, torch.bfloat16, stage0=staged, d0=4, ld0=4)
    key = id(w)
    assert staging.REGISTRY[key]["param"]() is w
    del w
    gc.collect()
    assert key not in staging.REGISTRY


def test_reused_id_does_not_hand_over_a_dead_parameters_entry():
    w = torch.nn.Parameter(torch.zeros(2, 2))
    staging.register(w, 1, torch.bfloat16, stage0=torch.zeros(2, 2, dtype=torch.bfloat16), d0=2, ld0=2)
    key = id(w)
    live = torch.nn.Parameter(torch.ones(2, 2))
    staging.REGISTRY[id(live)] = staging.REGISTRY[key]                 # what a reused id would find: the other parameter's entry
    assert staging.entry_of(live) is None and staging.entry_of(w) is not None
    staging.register(live, 1, torch.bfloat16, stage0=torch.ones(2, 2, dtype=torch.bfloat16), d0=2, ld0=2)
    assert staging.entry_of(live)["param"]() is live
    del w
    gc.collect()
    assert key not in staging.REGISTRY and staging.entry_of(live) is not None


def test_module_with_a_cache_and_registered_parameters_is_collectable():
    m = _Owner()
    m.staged("a", [m.ws[0]]); m.staged("heads", list(m.ws))
    ids = [id(p) for p in m.ws]
    assert all(i in staging.REGISTRY for i in ids)
    ref = weakref.ref(m)
    del m
    gc.collect()
    assert ref() is None and not any(i in staging.REGISTRY for i in ids)


def test_fewer_buffers_than_the_slot_holds_is_a_hit_and_more_keeps_the_first():
    """fc6 / fc7: the copy plus its transpose for training, the copy alone for a forward without backward"""
    w = torch.nn.Parameter(torch.ones(2, 3))
    cache, calls = staging.StageCache(), []
    both, one = ((2, 3), (3, 2)), ((2, 3),)

    def lookup(shapes):
        return cache.lookup("fc", (w,), shapes, torch.float32, w.device, lambda bufs: calls.append(len(bufs)))
    slot, built = lookup(both)
    a, b = slot.bufs
    assert built and calls == [2]
    slot, built = lookup(one)                                   # eval after train: nothing built, both buffers kept
    assert not built and calls == [2] and slot.bufs == (a, b)
    with torch.no_grad():
        w.add_(1.0)
    slot, built = lookup(one)                                   # a rebuild of the copy alone drops the transpose
    assert built and calls == [2, 1] and slot.bufs == (a,)
    slot, built = lookup(both)                                  # the transpose is wanted again: the copy stays where it is
    assert built and calls == [2, 1, 2] and slot.bufs[0] is a and tuple(slot.bufs[1].shape) == (3, 2) and cache.builds == 3


def test_copied_or_pickled_cache_starts_empty():
    """a copied module has new parameters: nothing of the original's slots (weak references, buffers) travels"""
    m = _Owner()
    m.staged("a", [m.ws[0]])
    twin = copy.deepcopy(m)
    assert list(twin.cache) == [] and twin.cache.builds == 0 and list(m.cache) == ["a"]
    again = pickle.loads(pickle.dumps(m.cache))
    assert isinstance(again, staging.StageCache) and list(again) == [] and again.builds == 0
    twin.staged("a", [twin.ws[0]])
    assert twin.cache.is_current("a") and twin.cache.buffers("a")[0].data_ptr() != m.cache.buffers("a")[0].data_ptr()


def test_entry_on_another_device_is_not_usable():
    w = torch.nn.Parameter(torch.zeros(2, 2))
    staging.register(w, 1, torch.bfloat16, stage0=torch.zeros(2, 2, dtype=torch.bfloat16, device="meta"), d0=2, ld0=2)
    assert staging.entry_of(w) is None
