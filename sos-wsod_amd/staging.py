"""Is this compute-dtype copy of a parameter still current?  Change tracking, the optimizer's registry of the copies it rewrites, and
the per-module `StageCache`.  Pure Python + torch: the staging kernels are launched by the callers' `build`."""
import weakref

import torch

_EPOCHS = [0, 0, 0]     # see epochs()


def params_written():
    """a kernel wrote parameters behind torch's version counters ("something changed": HipSGD, EMA, ...)"""
    _EPOCHS[0] += 1


def buffers_written():
    """a kernel wrote module BUFFERS behind torch's version counters (the Stage-3 teacher EMA)"""
    _EPOCHS[1] += 1


def invalidate_all():
    """every cached compute-dtype weight copy is stale (parameters were written wholesale behind the version counters: checkpoint
    load, re-homed parameter storage)"""
    _EPOCHS[0] += 1
    _EPOCHS[2] += 1


def epochs():
    """-> (parameter writes, buffer writes, wholesale invalidations) so far: a cache keyed on them is stale when one moved"""
    return tuple(_EPOCHS)


def mark_updated(p):
    """a kernel (HipSGD) has just rewritten THIS parameter behind torch's version counter: its own cached copies are stale unless
    the kernel rewrote them too and stamps them with the new key.  Per parameter: under the data-parallel trainer the update runs
    bucket by bucket, several calls per step — a global counter made every call invalidate the stamps of the buckets before it, and
    all but the last bucket's weights were re-staged in the next forward (12 staging launches and 0.3 ms per step)."""
    p.__dict__["_sw_epoch"] = _EPOCHS[0]


def param_key(p):
    """cache key of a parameter's current value (compute-dtype weight copies are rebuilt only when it changes): storage, torch's
    version counter, the epoch of the last wholesale invalidation and of the parameter's own last kernel update"""
    return (p.data_ptr(), p._version, _EPOCHS[2], p.__dict__.get("_sw_epoch", 0))


# ---------------------------------------------------------------------------------------------------- the optimizer's view
# id(parameter) -> dict(param, kind, dtype, stage0, stage1, d0, d1, d2, ld0, ld1, slots): the persistent copies HipSGD's fused
# step (sw_sgd_multi) rewrites from the freshly updated values, and the (slot, source index) pairs to re-stamp afterwards.
REGISTRY = {}


def register(p, kind, dtype, stage0=None, stage1=None, d0=0, d1=0, d2=0, ld0=0, ld1=0, slots=()):
    """The registry must not keep a model alive: the parameter is held weakly and its entry (with the staged copies) leaves when the
    parameter dies — a strong reference here leaked every deleted model's fc6 weight and its two bf16 copies (0.8 GB per VGG16
    detector; bench.py builds and drops six).  A slot holds its sources weakly too, and never its module."""
    key = id(p)

    def gone(ref):
        if REGISTRY.get(key, {}).get("param") is ref:          # (an id reused by a live parameter keeps ITS entry: another ref)
            del REGISTRY[key]
    REGISTRY[key] = dict(param=weakref.ref(p, gone), kind=kind, dtype=dtype, stage0=stage0, stage1=stage1, d0=d0, d1=d1, d2=d2,
                         ld0=ld0, ld1=ld1, slots=tuple(slots))


def entry_of(p):
    """the registered entry of `p` whose copies live on its device, or None"""
    ent = REGISTRY.get(id(p))
    if ent is None or ent["param"]() is not p or any(t is not None and t.device != p.device for t in (ent["stage0"], ent["stage1"])):
        return None
    return ent


def updated(p):
    """after the update kernel of `p`: the parameter has a new key, and the copies the kernel rewrote along with it are current
    under that key"""
    params_written()
    mark_updated(p)
    ent = entry_of(p)
    if ent is not None:
        for slot, j in ent["slots"]:
            slot.stamp(j, param_key(p))


# ---------------------------------------------------------------------------------------------------- the owning module's view
class Slot:
    """the buffers staged from a list of source parameters, and the key each source had when they were last written"""
    __slots__ = ("sources", "keys", "shapes", "where", "bufs")

    def stamp(self, j, pk):
        """source `j` now has key `pk`, and the buffers hold its value"""
        self.keys[j] = pk


class StageCache(dict):
    """One per owning module: name -> Slot."""
    builds = 0                      # misses so far (monotonic): constant across steady-state training steps

    def lookup(self, name, sources, shapes, dtype, device, build, alloc=torch.empty, reuse=True):
        """-> (slot, built).  shapes: one tuple per buffer (a tuple of tuples).  A hit — no source changed, and the slot's leading
        buffers have these shapes, dtype and device — launches nothing.  A miss calls build(buffers) on the current stream, writing
        into the tensors the slot already has wherever they fit (captured step graphs hold their addresses); the others come from
        alloc(*shape, dtype=, device=).  reuse=False: a miss never writes into an old buffer (an autograd node may have saved it)."""
        keys = [param_key(p) for p in sources]
        slot = self.get(name)
        held, old = (), ()
        if slot is not None and slot.where == (dtype, device):
            held, old = slot.shapes, slot.bufs
            if slot.keys == keys and held[:len(shapes)] == shapes:
                return slot, False
        bufs = tuple(old[i] if (reuse and held[i:i + 1] == (s,)) else alloc(*s, dtype=dtype, device=device) for i, s in enumerate(shapes))
        build(bufs)
        if slot is None:
            slot = self[name] = Slot()
        slot.sources, slot.keys = [weakref.ref(p) for p in sources], keys
        slot.shapes, slot.where, slot.bufs = shapes, (dtype, device), bufs
        self.builds += 1
        return slot, True

    def __reduce__(self):
        return StageCache, ()           # a copied or pickled module gets new parameters: its cache starts empty

    def is_current(self, name):
        return name in self and all(r() is not None and param_key(r()) == k for r, k in zip(self[name].sources, self[name].keys))

    def buffers(self, name):
        return self[name].bufs
