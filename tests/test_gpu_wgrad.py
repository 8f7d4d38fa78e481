"""GPU: the Stage-3 weight-gradient nodes (frcnn._LinearFn, _Conv3x3Fn, _Conv3x3LevelsFn, _BottleneckFn) over sos_wsod_amd.wgrad, each
configuration once inside a wgrad.grad_scope (queue + one grouped launch, or the add-in-the-epilogue path of an uncounted weight) and
once outside it (one launch per use, autograd sums), against float64 on the CPU from the same, already rounded operands:
dW = scale (.) sum over the uses of dy^T x, db = sum of dy.

Bar (derived, not chosen): n terms accumulated in f32 — products of bf16 operands are exact in f32, products of f32 operands
round once — in ANY order, then one multiply by the FrozenBN scale and the fold's last rounding: to first order
|got - ref| <= (n + 2) * 2^-24 * |scale| (.) (sum |dy|^T |x|) element by element.  Every check also asserts on the host that the
reference with one (non-empty) use left out violates that bar, so a lost use cannot pass."""
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
WORST = {}                      # node kind -> worst error / bound seen (printed per test)
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def fr():
    import sos_wsod_amd  # noqa: F401
    import sos_wsod_amd.frcnn as fr
    assert torch.cuda.is_available()
    return fr


def _rand(g, *shape, dtype):
    """unit-variance values, rounded to the compute dtype on the host (what every path and the reference then share)"""
    return torch.randn(*shape, generator=g).to(dtype).cuda()


def _d(t):
    return t.detach().cpu().double()


def _mm(dy, x):
    """one use of a 1x1 weight: (dy^T x, |dy|^T |x|) in float64"""
    dy, x = _d(dy), _d(x)
    return dy.t() @ x, dy.abs().t() @ x.abs()


def _conv(x, dz):
    """one use of a 3x3 weight (NHWC, stride 1, padding 1): (dW, the same sum over absolute values), (cout, cin, 3, 3) float64"""
    def one(x, dz):
        n, H, W, _ = x.shape
        xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
        out = torch.empty(dz.shape[3], x.shape[3], 3, 3, dtype=torch.float64)
        for ky in range(3):
            for kx in range(3):
                out[:, :, ky, kx] = torch.einsum("nhwo,nhwi->oi", dz, xp[:, ky:ky + H, kx:kx + W])
        return out
    x, dz = _d(x), _d(dz)
    return one(x, dz), one(x.abs(), dz.abs())


def _colsum(dy):
    dy = _d(dy).reshape(-1, dy.shape[-1])
    return dy.sum(0), dy.abs().sum(0)


def _check(kind, got, terms, n, scale=None):
    """got: the f32 gradient; terms: per use (value, magnitude) in float64, None for a use without rows; n: accumulated terms"""
    live = [t for t in terms if t is not None]
    ref, mag = sum(t[0] for t in live), sum(t[1] for t in live)
    s = torch.ones(ref.shape[0], dtype=torch.float64) if scale is None else _d(scale)
    s = s.view(-1, *([1] * (ref.dim() - 1)))
    ref, bound = ref * s, (n + 2) * U * mag * s.abs()
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape), (kind, got.shape, ref.shape)
    err = (_d(got) - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    WORST[kind] = max(WORST.get(kind, 0.0), ratio)
    assert bool((err <= bound).all()), (kind, ratio)
    for t in live:                                             # the bar can fail: a gradient that lost this use is outside it
        assert not bool(((t[0] * s).abs() <= bound).all()), kind


def _backward(fr, forward, params, mode):
    """forward() -> (outputs, their gradients).  mode "scope": forward and backward inside one grad_scope (uses counted);
    "uncounted": only the backward inside (the weights add to the first use's buffer in their epilogues); "plain": no scope.
    -> {parameter index: gradient}"""
    from sos_wsod_amd import wgrad
    for p in params:
        p.grad = None
    if mode == "scope":
        with wgrad.grad_scope():
            outs, gs = forward()
            torch.autograd.backward(outs, gs)
            wgrad.finish()
    elif mode == "uncounted":
        outs, gs = forward()
        with wgrad.grad_scope():
            torch.autograd.backward(outs, gs)
            wgrad.finish()
    else:
        outs, gs = forward()
        torch.autograd.backward(outs, gs)
    torch.cuda.synchronize()
    return {i: p.grad for i, p in enumerate(params) if p.grad is not None}


def _same_shape(a, b, params):
    assert set(a) == set(b) == set(range(len(params))), (sorted(a), sorted(b))
    assert all(a[i].shape == b[i].shape == params[i].shape for i in a)


# ------------------------------------------------------------------------------------------------------------- linear
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("with_scale", [False, True], ids=["bias", "frozenbn"])
@pytest.mark.parametrize("splits,rows,modes", [
    ((64,), (1024, 0, 96), ("scope", "plain")),              # 1024: the smallest P at which wgrad_1x1 splits K; 0: an arrival without rows
    ((3, 12), (1024, 0, 96), ("scope", "plain")),            # packed: ld = 16 with a pad row, two parameters in one buffer
    ((64,), (0, 0), ("scope", "plain")),                     # nobody brings rows: the last arrival zero-fills
    ((64,), (96,), ("scope", "plain")),                      # a single use inside a scope: not queued
    # an uncounted key: the use that runs second (the one created FIRST) adds to the registered buffer in its epilogue —
    ((64,), (1024, 96), ("uncounted", "plain")),             # through the K-split fold with the buffer as residual,
    ((64,), (96, 1024), ("uncounted", "plain")),             # and as ONE slab (which needs the split-K workspace for the row scale)
    ((3, 12), (96, 1024), ("uncounted", "plain")),
], ids=["three", "packed", "empty", "single", "uncounted-split", "uncounted-oneslab", "uncounted-packed"])
def test_linear_node(fr, dtype, with_scale, splits, rows, modes):
    g = torch.Generator().manual_seed(5)
    D, out_f = 64, sum(splits)
    ld = (out_f + 7) // 8 * 8
    ws = [torch.nn.Parameter(_rand(g, n, D, dtype=torch.float32)) for n in splits]
    bs = [] if with_scale else [torch.nn.Parameter(_rand(g, n, dtype=torch.float32)) for n in splits]
    scale = (torch.rand(out_f, generator=g) + 0.5).cuda() if with_scale else None
    staged = torch.zeros(ld, D, device="cuda", dtype=dtype)
    staged[:out_f] = (torch.cat([w.detach() for w in ws]) * (1.0 if scale is None else scale[:, None])).to(dtype)
    bias = torch.zeros(ld, device="cuda") if with_scale else torch.cat([b.detach() for b in bs] + [torch.zeros(ld - out_f, device="cuda")])
    xs = [_rand(g, P, D, dtype=dtype) for P in rows]
    gys = [_rand(g, P, out_f, dtype=dtype) for P in rows]
    params = ws + bs

    def forward():
        return [fr._LinearFn.apply(x, staged, bias, scale, False, False, splits, None, *params) for x in xs], gys
    n = sum(rows)
    wt = [_mm(gy, x) if x.shape[0] else None for gy, x in zip(gys, xs)]
    bt = [_colsum(gy) if gy.shape[0] else None for gy in gys]
    res = [_backward(fr, forward, params, m) for m in modes]
    _same_shape(res[0], res[1], params)
    for got in res:
        r0 = 0
        for i, k in enumerate(splits):
            if n == 0:
                assert not bool(got[i].any()) and (with_scale or not bool(got[len(splits) + i].any()))
            else:
                cut = lambda t: None if t is None else (t[0][r0:r0 + k], t[1][r0:r0 + k])
                _check("linear", got[i], [cut(t) for t in wt], n, None if scale is None else scale[r0:r0 + k])
                if not with_scale:
                    _check("bias", got[len(splits) + i], [cut(t) for t in bt], n)
            r0 += k
    print("worst error / bound:", {k: "%.2f" % v for k, v in WORST.items()})


# ------------------------------------------------------------------------------------------------------------- 3x3
def _staged3x3(w, scale, dtype):
    weff = w.detach() * (1.0 if scale is None else scale.view(-1, 1, 1, 1))
    return (weff.permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1]).to(dtype).contiguous(),
            weff.flip(2, 3).permute(1, 2, 3, 0).reshape(w.shape[1], 9, w.shape[0]).to(dtype).contiguous())


_BIG, _SMALL = [(2, 16, 24), (1, 8, 12)], [(1, 4, 6), (2, 2, 3)]          # grouped 256x256-tile kernel / the few-pixel kernel (small_map)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("with_scale", [False, True], ids=["bias", "frozenbn"])
@pytest.mark.parametrize("maps,modes", [
    (_BIG + _SMALL, ("scope", "plain")),                     # backward arrives in reverse: small maps first, the flush runs big then small
    (_SMALL + _BIG, ("scope", "plain")),
    (_SMALL, ("scope", "plain")),                            # all small: the first small launch overwrites
    (_BIG[:1], ("scope", "plain")),                          # a single use
    ([_BIG[0], _SMALL[0]], ("uncounted", "plain")),          # uncounted key: the use that runs second (a big map) adds in its fold
    ([_SMALL[0], _BIG[0]], ("uncounted", "plain")),          # ... the use that runs second is a small map
], ids=["big-small", "small-big", "all-small", "single", "uncounted-big", "uncounted-small"])
def test_conv3x3_node(fr, dtype, with_scale, maps, modes):
    from sos_wsod_amd import wgrad
    assert [wgrad.small_map(H, W) for _, H, W in _BIG + _SMALL] == [False, False, True, True]
    g = torch.Generator().manual_seed(7)
    C = 64
    w = torch.nn.Parameter(_rand(g, C, C, 3, 3, dtype=torch.float32))
    b = None if with_scale else torch.nn.Parameter(_rand(g, C, dtype=torch.float32))
    scale = (torch.rand(C, generator=g) + 0.5).cuda() if with_scale else None
    st, std = _staged3x3(w, scale, dtype)
    bias = torch.zeros(C, device="cuda") if b is None else b.detach()
    xs = [_rand(g, n, H, W, C, dtype=dtype) for n, H, W in maps]
    gys = [_rand(g, n, H, W, C, dtype=dtype) for n, H, W in maps]
    params = [w] + ([] if b is None else [b])

    def forward():
        return [fr._Conv3x3Fn.apply(x, st, std, bias, scale, False, w, b) for x in xs], gys
    n = sum(a * H * W for a, H, W in maps)
    wt, bt = [_conv(x, gy) for x, gy in zip(xs, gys)], [_colsum(gy) for gy in gys]
    res = [_backward(fr, forward, params, m) for m in modes]
    _same_shape(res[0], res[1], params)
    for got in res:
        _check("conv3x3", got[0], wt, n, scale)
        if b is not None:
            _check("bias", got[1], bt, n)
    print("worst error / bound:", {k: "%.2f" % v for k, v in WORST.items()})


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_conv3x3_levels_node_one_weight_on_five_levels(fr, dtype):
    import sos_wsod_amd.ops as ops
    g = torch.Generator().manual_seed(9)
    C = 64
    maps = [(1, 16, 24), (1, 8, 12), (1, 4, 6), (1, 2, 3), (2, 2, 2)]
    conv = fr.Conv(C, C, 3).cuda()
    with torch.no_grad():
        conv.bias.copy_(_rand(g, C, dtype=torch.float32))
    ops.StagePlan(conv._stage_entries(dtype), dtype).run()
    xs = [_rand(g, n, H, W, C, dtype=dtype) for n, H, W in maps]
    gys = [_rand(g, n, H, W, C, dtype=dtype) for n, H, W in maps]
    params = [conv.weight, conv.bias]

    def forward():
        return list(fr._conv3x3_levels([conv] * len(maps), xs)), gys
    n = sum(a * H * W for a, H, W in maps)
    wt, bt = [_conv(x, gy) for x, gy in zip(xs, gys)], [_colsum(gy) for gy in gys]
    res = [_backward(fr, forward, params, m) for m in ("scope", "plain")]
    _same_shape(res[0], res[1], params)
    for got in res:
        _check("conv3x3", got[0], wt, n)
        _check("bias", got[1], bt, n)
    print("worst error / bound:", {k: "%.2f" % v for k, v in WORST.items()})


# ------------------------------------------------------------------------------------------------------------- bottleneck
class _Operands:
    """what the bottleneck node hands the weight-gradient producers, per parameter: the node's operands are its own intermediate
    activations and gradients, so the reference takes them from the calls (frcnn reaches wgrad.join / wgrad_1x1 / wgrad_3x3 through the
    module at call time)"""

    def __init__(self, monkeypatch, wgrad, blk):
        self.uses = {}                                          # id(parameter) -> [(dy, x), ...]
        ones = [blk.conv1.weight, blk.conv3.weight] + ([] if blk.shortcut is None else [blk.shortcut.weight])
        real_join, real_1x1, real_3x3 = wgrad.join, wgrad.wgrad_1x1, wgrad.wgrad_3x3

        def join(key, operands, *a, **k):
            got = real_join(key, operands, *a, **k)
            if got is not wgrad.NOT_QUEUED and isinstance(key, tuple):       # (wgrad_3x3 joins too, under the parameter's id: recorded below)
                assert key == ("1x1", id(ones[0]))
                for w, pair in zip(ones, operands):
                    self.uses.setdefault(id(w), []).append(pair)
            return got

        def one(gs, x, scale, key=None):
            self.uses.setdefault(key, []).append((gs, x))
            return real_1x1(gs, x, scale, key)

        def three(x4, dz4, scale, key=None):
            self.uses.setdefault(key, []).append((dz4, x4))
            return real_3x3(x4, dz4, scale, key)
        monkeypatch.setattr(wgrad, "join", join); monkeypatch.setattr(wgrad, "wgrad_1x1", one); monkeypatch.setattr(wgrad, "wgrad_3x3", three)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("cin,stride", [(64, 2), (128, 1)], ids=["shortcut-stride2", "identity"])
@pytest.mark.parametrize("lockstep", [False, True], ids=["two-passes", "two-maps-one-call"])
def test_bottleneck_node(fr, monkeypatch, dtype, cin, stride, lockstep):
    import sos_wsod_amd.ops as ops
    from sos_wsod_amd import wgrad
    g = torch.Generator().manual_seed(11)
    mid, cout = 32, 128
    blk = fr.BottleneckBlock(cin, cout, mid, stride).cuda()
    assert (blk.shortcut is None) == (cin == cout)
    convs = [blk.conv1, blk.conv2, blk.conv3] + ([] if blk.shortcut is None else [blk.shortcut])
    with torch.no_grad():
        for c in convs:
            c.norm.weight.copy_(torch.rand(c.norm.weight.shape, generator=g) + 0.5)
            c.norm.running_var.copy_(torch.rand(c.norm.weight.shape, generator=g) + 0.5)
            c.weight.copy_(torch.randn(c.weight.shape, generator=g) / (c.weight[0].numel() ** 0.5))
    ops.StagePlan([e for c in convs for e in c._stage_entries(dtype)], dtype).run()
    params = [c.weight for c in convs]
    maps = [(1, 12, 16), (1, 8, 10)]
    xs = [_rand(g, n, H, W, cin, dtype=dtype) for n, H, W in maps]
    out_maps = [(n, (H + stride - 1) // stride, (W + stride - 1) // stride) for n, H, W in maps]
    gys = [_rand(g, n, H, W, cout, dtype=dtype) for n, H, W in out_maps]

    def forward():
        if lockstep:                                            # the rows of both maps in ONE call: one counted use, forced into the queue
            rows = torch.cat([x.reshape(-1, cin) for x in xs])
            return [fr._BottleneckFn.apply(rows, (blk, maps), *params)], [torch.cat([gy.reshape(-1, cout) for gy in gys])]
        return [blk(x) for x in xs], gys
    n = sum(a * H * W for a, H, W in out_maps)
    res = []
    for mode in ("scope", "plain"):
        rec = _Operands(monkeypatch, wgrad, blk)
        got = _backward(fr, forward, params, mode)
        monkeypatch.undo()
        for i, c in enumerate(convs):
            uses = rec.uses[id(c.weight)]
            assert len(uses) == (2 if c.k == 3 or not lockstep else 1), (mode, i, len(uses))
            terms = [_conv(x, dy) if c.k == 3 else tuple(t.view(*t.shape, 1, 1) for t in _mm(dy, x)) for dy, x in uses]
            _check("bottleneck conv2" if c.k == 3 else "bottleneck 1x1", got[i], terms, n, _staged_scale(fr, c))
        res.append(got)
    _same_shape(res[0], res[1], params)
    print("worst error / bound:", {k: "%.2f" % v for k, v in WORST.items()})


def _staged_scale(fr, conv):
    return fr._staged_of(conv).scale
