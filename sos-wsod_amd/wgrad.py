"""Weight gradients of parameters that are used several times per iteration: ONE buffer per parameter, summed in the kernels
(`grad_scope`, `join`), the producers behind it and the split planners of the grouped launches, which the Stage-1 backbone shares.
Pure Python + torch; every kernel goes through `ops`.

What autograd is handed is always a VIEW (a tensor object of its own) on a buffer's storage, never the object the scope keeps: the
accumulator of a parameter adopts a gradient without copying it only when nobody else holds the tensor object it was handed (18
device-to-device copies per Stage-3 iteration otherwise)."""
import torch

from . import ops

_SCOPE = None                   # the active grad_scope (or None)
_CALLER_GRAD_ENABLED = True     # grad mode of the code that called the running CountedFunction.apply (see there)
NOT_QUEUED = object()           # join's answer when the caller has to compute its gradient one by one


class _Queue:
    """one counted key: the f32 buffers autograd holds, the FrozenBN scales, the operands of the uses so far, the uses still to come"""
    __slots__ = ("bufs", "scales", "uses", "left")


class grad_scope:
    """Wrap the forward passes AND the one `backward()` call of an iteration whose graph uses parameters more than once (the Stage-3
    student: two forward passes per iteration, unbias/ubteacher/engine/trainer.py:527-538; the RPN head's convolution on five FPN
    levels in each) — autograd would add the uses' weight gradients with a torch kernel per parameter.  Inside the scope
      * the first weight-gradient node of a parameter registers the buffer it returns (`note_grad`) and every later node of the same
        parameter ADDS to that buffer inside its own fold / GEMM epilogue (`pending_grad`) and returns no gradient;
      * a forward pass counts the uses of a weight (`count_use`); its weight-gradient nodes then only QUEUE their operands and the
        last of them runs all of them as one grouped launch + one fold (`join`).
    The accumulator node of a parameter runs after all of its incoming edges (every use), on the same stream, so it sees the
    finished sum; the data-parallel reducer's hooks hang on that node and are therefore not affected.  A counted use whose
    backward node never runs leaves a queued gradient unfinished (uninitialised memory): `finish` — call it between `backward()`
    and `optimizer.step()` — and __exit__ raise then.  Outside a scope every helper is inert: plain autograd behaviour."""

    def __enter__(self):
        global _SCOPE
        self._prev, _SCOPE = _SCOPE, self
        self._bufs, self._uses, self._queues = {}, {}, {}
        return self

    def _check(self, loud=True, clear=False):
        left = sum(1 for q in self._queues.values() if q.uses)
        if left or clear:
            self._bufs, self._uses, self._queues = {}, {}, {}
        if left and loud:
            raise RuntimeError(f"grad_scope: {left} queued weight gradient(s) were never finished — a use counted in the forward pass "
                               "did not take part in backward(); run this graph without wgrad.grad_scope")

    def __exit__(self, exc_type, *exc):
        global _SCOPE
        _SCOPE = self._prev
        self._check(loud=exc_type is None, clear=True)


def active():
    return _SCOPE


def use_count(key):
    return 0 if _SCOPE is None else _SCOPE._uses.get(key, 0)


def finish():
    """raise if a queued weight gradient was never run, BEFORE the optimizer applies it (the scope is left empty then)"""
    if _SCOPE is not None:
        _SCOPE._check()


class CountedFunction(torch.autograd.Function):
    """torch.autograd.Function whose forward may call `count_use`.  Inside `forward` autograd has ALREADY switched grad mode off —
    whether the caller ran under torch.no_grad() or not — and ctx.needs_input_grad stays True for a parameter that requires grad:
    the only place that still sees the caller's mode is `apply` itself, so it is recorded there.  (torch.is_grad_enabled() inside
    count_use is always False: nothing was counted, every Stage-3 weight gradient silently ran one by one, 16.2 -> 17.3 ms.)"""

    @classmethod
    def apply(cls, *args, **kwargs):
        global _CALLER_GRAD_ENABLED
        prev, _CALLER_GRAD_ENABLED = _CALLER_GRAD_ENABLED, torch.is_grad_enabled()
        try:
            return super().apply(*args, **kwargs)
        finally:
            _CALLER_GRAD_ENABLED = prev


def count_use(key):
    """inside a CountedFunction.forward: this pass contributes one weight-gradient node for `key` (not under no_grad: no node)"""
    if _SCOPE is not None and key is not None and _CALLER_GRAD_ENABLED:
        _SCOPE._uses[key] = _SCOPE._uses.get(key, 0) + 1


def pending_grad(key, shape):
    """the f32 buffer an earlier node of this backward pass registered for `key` (viewed as `shape`), or None"""
    if _SCOPE is None or key is None:
        return None
    buf = _SCOPE._bufs.get(key)
    if buf is None or buf.numel() != int(torch.Size(shape).numel()) or not buf.is_contiguous():
        return None
    return buf.view(shape)


def note_grad(key, buf):
    """register `buf` for `key`: the scope keeps an alias, the caller hands autograd a view of its own"""
    if _SCOPE is not None and key is not None:
        _SCOPE._bufs[key] = buf.view(buf.shape)


def join(key, operands, shapes, scales, device, flush, force=False):
    """One weight-gradient node's arrival at the queue of `key`.  NOT_QUEUED (the caller computes its gradient itself) without a
    scope or key, or when fewer than two uses were counted (`force`: one is enough — several maps in one call).  Else the first
    arrival allocates the f32 buffers (`shapes`) and stores `scales`, every arrival appends its `operands` (None: no rows), the last
    calls flush(bufs, scales, [operands, ... in arrival order]) once — or zero-fills when nobody brought operands.
    -> views of the buffers for the first arrival, None for the others."""
    sc = _SCOPE
    if sc is None or key is None:
        return NOT_QUEUED
    n = sc._uses.get(key, 0)
    if n < 2 and not (force and n == 1):
        return NOT_QUEUED
    q = sc._queues.get(key)
    first = q is None
    if first:
        q = sc._queues[key] = _Queue()
        q.bufs, q.scales, q.uses, q.left = [torch.empty(s, device=device, dtype=torch.float32) for s in shapes], scales, [], n
    if operands is not None:
        q.uses.append(operands)
    q.left -= 1
    if q.left == 0:
        if q.uses:
            flush(q.bufs, q.scales, q.uses)
            q.uses = []
        else:
            for b in q.bufs:
                b.zero_()
    return [b.view(b.shape) for b in q.bufs] if first else None


PLAN_CACHE = {}


def _cached(key, value):
    if len(PLAN_CACHE) > 512:
        PLAN_CACHE.clear()
    PLAN_CACHE[key] = value
    return value


def wgrad_grouped_target(shapes, bk, n_cu=256, candidates=(40, 48, 56, 64, 72, 80, 96, 112, 128, 160)):
    """K-tiles per work item of the grouped weight-gradient launch for this set of problems.  shapes: [(npix, cout, n_cols)].
    The launch deals the item list round-robin to n_cu resident workgroups, so its length is the busiest workgroup's sum of
    K-tiles: simulated here for a few targets (plus the extra slab traffic of more K-splits, priced at ~25 K-tile-times per
    extra slab of a 512 x 4608 gradient) and the cheapest kept.  Cached per shape set: the schedule of a training run's view
    sizes is computed once."""
    key = (tuple(shapes), bk, n_cu, candidates)
    hit = PLAN_CACHE.get(key)
    if hit is not None:
        return hit
    best = None
    for T in candidates:
        load = [0.0] * n_cu
        t, slabs = 0, 0.0
        for npix, cout, ncols in shapes:
            ktiles = (npix + bk - 1) // bk
            ns = max(1, (ktiles + T // 2) // T)
            per = (ktiles + ns - 1) // ns
            ntile = ((cout + 255) // 256) * ((ncols + 255) // 256)
            for _ in range(ns * ntile):
                load[t % n_cu] += per
                t += 1
            slabs += (ns - 1) * cout * ncols / (512.0 * 4608.0)
        cost = max(load) + 25.0 * slabs / max(1, n_cu // 32)
        if best is None or cost < best[0]:
            best = (cost, T)
    return _cached(key, best[1])


def wgrad_grouped_splits(npix, bk, target_ktiles):
    """K-splits of one (layer, view batch) problem of the grouped weight-gradient launch: work items of ~target_ktiles K-tiles
    each, so that the 256x256 items of all layers are of similar length (conv3 maps hold 4x the pixels of conv4 / conv5)"""
    ktiles = (npix + bk - 1) // bk
    return max(1, (ktiles + target_ktiles // 2) // target_ktiles)


def wgrad_direct_covers(probs, dtype):
    """the shape conditions of the direct weight-gradient kernel (csrc/conv_wgrad_direct.hip, sw_conv3x3_wgrad_direct_try): every
    problem (n, H, W, cin, cout, dil) of a grouped launch must meet them, else the whole list runs as implicit GEMMs"""
    if dtype != torch.bfloat16:
        return False
    return all(cout % 64 == 0 and cin % 64 == 0 and dil in (1, 2) and H >= 8 and n * ((W + 31) // 32) * H >= 8
               for n, H, W, cin, cout, dil in probs)


def wgrad_nslab(npix, nsplit, bk=64):
    """slabs sw_conv3x3_wgrad_workspace_floats(..., splitk = nsplit) stands for (the K range of a split is a multiple of bk pixels)"""
    kps = -(-(-(-npix // max(1, nsplit))) // bk) * bk
    return -(-npix // kps)


def wgrad_direct_splits(probs, n_slots=512, candidates=(160, 192, 224, 256, 320, 384, 448, 512)):
    """pixel splits per problem for the direct weight-gradient kernel.  Its work items are (problem, split, 64 x 64 channel block), all of
    one problem equally long (steps = image rows of 32-pixel strips); the resident workgroups (two per CU) take the item list round-robin.
    For a few target item lengths: simulate that deal (plus ~6 steps of prologue / epilogue per item; a CU's two workgroups share its
    matrix pipes — ~1 us per step each side by side, ~0.6 us for one alone) and price the slabs (written by the kernel, read by the
    fold: ~0.25 us per MB) — keep the cheapest.  Measured (tools/wgrad_shapes.py, headline / recipe / COCO shape sets): 300-400 steps per
    item is the flat optimum, shorter items pay in slab traffic, one item per block loses the L2 sharing of a pixel range.  Cached per
    shape set."""
    key = ("direct", tuple(probs), n_slots, candidates)
    hit = PLAN_CACHE.get(key)
    if hit is not None:
        return hit
    best = None
    for S in candidates:
        load = [0.0] * n_slots
        t, mb, ns_list = 0, 0.0, []
        for n, H, W, cin, cout, dil in probs:
            steps = n * ((W + 31) // 32) * H
            ns = max(1, min(int(steps / S + 0.5), steps // 8))
            eff = wgrad_nslab(n * H * W, ns)
            while eff > 1 and -(-steps // eff) < 8:
                ns -= 1
                eff = wgrad_nslab(n * H * W, ns)
            per = -(-steps // eff)
            ns_list.append(ns)
            for _ in range(eff * (cout // 64) * (cin // 64)):
                load[t % n_slots] += per + 6
                t += 1
            mb += eff * cout * 9 * cin * 4e-6
        half = n_slots // 2
        busiest = max(min(load[c], load[c + half]) + 0.6 * abs(load[c] - load[c + half]) for c in range(half))
        cost = busiest + 0.25 * mb
        if best is None or cost < best[0]:
            best = (cost, ns_list)
    return _cached(key, best[1])


# ====================================================================================================== producers
GROUP_TARGETS = (8, 12, 16, 24, 32, 40, 48, 56, 64, 72, 80, 96, 112, 128, 160)      # K-tiles per work item tried for a grouped launch
GROUP_TARGETS_1X1 = (4, 6) + GROUP_TARGETS


def eff_splits(K, sk, bf16):
    """the K-split count sw_gemm will really use (gemm.hip effective_splits)"""
    bk = 64 if bf16 else 32
    kps = -(-K // max(1, sk))
    kps = -(-kps // bk) * bk
    return -(-K // kps)


def wgrad_1x1(gs, x, scale, key=None):
    """dW (out, in) f32 = scale[:, None] * gs^T x over the pixels: K-split slabs + ordered fold (deterministic).  Inside a
    grad_scope a second use of the same weight (`key`) adds to the first use's buffer in the fold / epilogue and returns None
    (ALWAYS, once a buffer is registered: autograd may already have replaced the registered tensor by a sum of its own if a later
    use handed it a gradient too).  The callers hand autograd views (row blocks) of what this returns."""
    P, ld = gs.shape
    D = x.shape[1]
    tiles = ((ld + 127) // 128) * ((D + 127) // 128)
    sk = max(1, min(64, 512 // tiles, P // 512))
    prev = pending_grad(key, (ld, D))
    if prev is not None:
        ws = None
        if scale is not None and eff_splits(P, sk, gs.dtype == torch.bfloat16) == 1:
            ws = torch.empty(ld * D, device=gs.device, dtype=torch.float32)        # one slab: row scale + residual run in the fold
        ops.gemm(gs, x, prev, ld, D, P, a_kstrided=True, b_kstrided=True, splitk=sk,
                 ep=ops.make_epilogue(out_dtype=torch.float32, row_scale=scale, residual=prev, splitk_workspace=ws))
        return None
    dw = torch.empty(ld, D, device=gs.device, dtype=torch.float32)
    ep = None if scale is None else ops.make_epilogue(out_dtype=torch.float32, row_scale=scale)
    ops.gemm(gs, x, dw, ld, D, P, a_kstrided=True, b_kstrided=True, splitk=sk, ep=ep)
    note_grad(key, dw)
    return dw


def bias_grad(gs2d, n, key=None):
    """db (n,) f32 = column sums of the (masked) output gradient; grad_scope as wgrad_1x1 (key: the bias parameter)"""
    P = gs2d.shape[0]
    prev = pending_grad(key, (n,))
    if prev is not None:
        if P > 0:
            ops.colsum(gs2d, P, n, prev, accumulate=True)
        return None
    db = torch.empty(n, device=gs2d.device, dtype=torch.float32)
    if P > 0:
        ops.colsum(gs2d, P, n, db)
    else:
        db.zero_()
    note_grad(key, db)
    return db.view(n)


def flush_wgrad_1x1(bufs, scales, uses):
    """join's flush for 1x1 weights.  uses: per arrival one (A (P, M), B (P, N)) pair per buffer — a bottleneck block's (dh1, x),
    (gs, h2)[, (gs, x)], a linear layer's (gs, x); bufs[w] (M, N[, 1, 1]) = scales[w][:, None] * sum over the uses of A^T B: ONE
    sw_gemm_kk_grouped launch and ONE sw_splitk_fold_multi"""
    dtype = uses[0][0][0].dtype
    bk = 64 if dtype == torch.bfloat16 else 32
    shapes = [(a.shape[0], a.shape[1], b.shape[1]) for use in uses for a, b in use]
    target = wgrad_grouped_target(shapes, bk, candidates=GROUP_TARGETS_1X1)
    probs, folds = [], []
    for w, (buf, scale) in enumerate(zip(bufs, scales)):
        ns = [wgrad_grouped_splits(use[w][0].shape[0], bk, target) for use in uses]
        nsl = [ops.gemm_kk_nslab(dtype, use[w][0].shape[0], s_) for use, s_ in zip(uses, ns)]
        ws = torch.empty(sum(nsl), buf.numel(), device=buf.device, dtype=torch.float32)
        off = 0
        for use, s_, k in zip(uses, ns, nsl):
            probs.append((use[w][0], use[w][1], ws[off:], s_))
            off += k
        folds.append((ws, sum(nsl), buf, scale, False))
    ops.gemm_kk_grouped(probs)
    ops.splitk_fold_multi(folds)


def small_map(H, W):
    """maps of a few pixels (p5 / p6 of small images: 4x4, 2x2) are below the gathering loader's tile geometry (sw_conv3x3_wgrad
    returns -6): a direct kernel, one thread per (co, ci), takes them"""
    return (64 // W) + 1 > 2 * H


def flush_wgrad_3x3(bufs, scales, uses):
    """join's flush for one 3x3 weight.  uses: the (x, dy) pairs: ONE grouped 256x256-tile launch (sw_conv3x3_wgrad_grouped: every
    pair's K-splits as work items of one resident grid) + ONE fold over all slabs (x FrozenBN scale) into the buffer autograd already
    holds.  Measured (tools/probes/stage3_grouped_wgrad_probe.py): the RPN head's 10 uses 641 -> 383 us, an FPN output convolution's
    two 330 -> 256 (p2) / 71 -> 46 (p4), res5 conv2 83 -> 48, res3 conv2 74 -> 52."""
    dw, scale = bufs[0], scales[0]
    cout, cin = dw.shape[:2]
    big = [(x, dz) for x, dz in uses if not small_map(x.shape[1], x.shape[2])]
    small = [(x, dz) for x, dz in uses if small_map(x.shape[1], x.shape[2])]
    wrote = False
    if big:
        bk = 64 if big[0][0].dtype == torch.bfloat16 else 32
        shapes = [(x.shape[0] * x.shape[1] * x.shape[2], cout, 9 * cin) for x, _ in big]
        target = wgrad_grouped_target(shapes, bk, candidates=GROUP_TARGETS)
        splits = [wgrad_grouped_splits(sh[0], bk, target) for sh in shapes]
        nsl = [ops.conv3x3_wgrad_nslab(x, cout, sp) for (x, _), sp in zip(big, splits)]
        ws = torch.empty(sum(nsl), cout * 9 * cin, device=dw.device, dtype=torch.float32)
        off, items = 0, []
        for (x, dz), sp, n in zip(big, splits, nsl):
            items.append((x, dz, ws[off:], 1, sp))
            off += n
        ops.conv3x3_wgrad_grouped(items)
        ops.conv3x3_wgrad_fold(ws, sum(nsl), dw, cout_scale=scale)
        wrote = True
    for x, dz in small:
        ops.conv3x3_wgrad_small(x, dz, dw, cout_scale=scale, accumulate=wrote)
        wrote = True


def wgrad_3x3(x4, dz4, scale, key=None):
    """dW (cout, cin, 3, 3) f32 of a 3x3 convolution (sw_conv3x3_wgrad: slabs + fold, x FrozenBN scale).  Inside a grad_scope: a
    weight whose uses were counted queues its (x, dy) pairs and the LAST use computes all of them at once (flush_wgrad_3x3) into the
    buffer the first use handed to autograd; an uncounted weight adds to the first use's buffer in the fold, as wgrad_1x1 does."""
    n, H, W, cin = x4.shape
    cout = dz4.shape[3]
    got = join(key, (x4, dz4), ((cout, cin, 3, 3),), (scale,), x4.device, flush_wgrad_3x3)
    if got is not NOT_QUEUED:
        return None if got is None else got[0]
    prev = pending_grad(key, (cout, cin, 3, 3))
    dw = prev if prev is not None else torch.empty(cout, cin, 3, 3, device=x4.device, dtype=torch.float32)
    if small_map(H, W):
        ops.conv3x3_wgrad_small(x4, dz4, dw, cout_scale=scale, accumulate=prev is not None)
    else:
        tiles = ((cout + 127) // 128) * ((9 * cin + 127) // 128)
        sk = max(1, min(32, 512 // tiles, max(1, n * H * W // 1024)))
        ops.conv3x3_wgrad(x4, dz4, dw, 1, splitk=sk, cout_scale=scale, accumulate=prev is not None)
    if prev is not None:
        return None
    note_grad(key, dw)
    return dw.view(cout, cin, 3, 3)
