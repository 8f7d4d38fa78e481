"""Compare what two builds of the library compute, array by array, on the GPU tests themselves.

As a pytest plugin it wraps every public function of sos_wsod_amd.ops: after each call, every CUDA tensor among the arguments and in the
result is checksummed on the device (a position-weighted 64-bit sum over the tensor's words: any changed word changes it) and
(test id, function, argument path, shape, dtype, checksum) is appended to $OPS_CHECKSUM_OUT.  Calls made while a stream is capturing are
skipped.  Run the same tests once per library, then compare:

  SW_LIB_PATH=$PWD/sos-wsod_amd/libsoswsod_hip_base.so OPS_CHECKSUM_OUT=a.json PYTHONPATH=tools python -m pytest -p ops_checksum -m gpu tests/...
  OPS_CHECKSUM_OUT=b.json PYTHONPATH=tools python -m pytest -p ops_checksum -m gpu tests/...
  python tools/ops_checksum.py a.json b.json

Arrays that differ between two runs of ONE library (f32 atomics, inputs drawn without a seed, torch.empty outputs seen before they are
written) show up when a is compared with a second run of a."""
import collections
import functools
import json
import os
import sys
import types

_records, _current, _patched = [], [""], [False]


def _tensors(x, path, out, depth=0):
    import torch
    if isinstance(x, torch.Tensor):
        out.append((path, x))
    elif depth < 4 and isinstance(x, (list, tuple)):
        for i, y in enumerate(x):
            _tensors(y, f"{path}.{i}", out, depth + 1)
    elif depth < 4 and isinstance(x, dict):
        for k, y in x.items():
            _tensors(y, f"{path}.{k}", out, depth + 1)


def _checksum(t):
    import torch
    v = t.detach().contiguous().reshape(-1).clone()          # a fresh allocation: storage offset 0
    if v.numel() == 0:
        return 0
    nb = v.numel() * v.element_size()
    v = v.view(torch.uint8)
    v = v.view(torch.int32) if nb % 4 == 0 else (v.view(torch.int16) if nb % 2 == 0 else v)
    total = 0
    for lo in range(0, v.numel(), 1 << 26):
        c = v[lo:lo + (1 << 26)].long()
        w = (torch.arange(lo, lo + c.numel(), device=v.device, dtype=torch.int64) * 2654435761) % 2147483647 + 1
        total = (total + int((c * w).sum().item())) & 0xFFFFFFFFFFFFFFFF
    return total


def _wrap(name, fn):
    import torch

    @functools.wraps(fn)
    def w(*a, **k):
        r = fn(*a, **k)
        if torch.cuda.is_current_stream_capturing():
            return r
        ts = []
        _tensors(a, "a", ts); _tensors(k, "k", ts); _tensors(r, "r", ts)
        torch.cuda.synchronize()
        for path, t in ts:
            if t.is_cuda:
                _records.append([_current[0], name, path, list(t.shape), str(t.dtype), _checksum(t)])
        return r
    return w


def pytest_runtest_setup(item):
    _current[0] = item.nodeid
    if not _patched[0]:
        _patched[0] = True
        import sos_wsod_amd.ops as ops
        for name, fn in list(vars(ops).items()):
            if isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not name.startswith("_"):
                setattr(ops, name, _wrap(name, fn))


def pytest_sessionfinish(session, exitstatus):
    if os.environ.get("OPS_CHECKSUM_OUT"):
        with open(os.environ["OPS_CHECKSUM_OUT"], "w") as f:
            json.dump(_records, f)


def compare(pa, pb):
    a, b = (json.load(open(p)) for p in (pa, pb))
    if [r[:5] for r in a] != [r[:5] for r in b]:
        print(f"the two runs did not make the same calls ({len(a)} and {len(b)} arrays)")
        return 1
    diff = collections.Counter((x[0], x[1]) for x, y in zip(a, b) if x[5] != y[5])
    print(f"{len(a)} arrays compared, {sum(diff.values())} differ")
    print("per file:", dict(collections.Counter(r[0].split("::")[0] for r in a)))
    print("per function:", dict(collections.Counter(r[1] for r in a)))
    for (test, fn), n in diff.items():
        print("differ:", n, fn, test)
    return 0


if __name__ == "__main__":
    sys.exit(compare(sys.argv[1], sys.argv[2]))
