"""Thin torch-tensor wrappers over the C-ABI kernels (include/soswsod_hip.h).

torch is used here only for device memory and the current HIP stream; every computation is a
hand-written gfx950 kernel.  All tensors must live on the GPU and be contiguous where stated.
"""
import ctypes

import torch

from ._lib import SW_BF16, SW_F32, Epilogue, check, lib


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _splitmix64(x):
    """sw_splitmix64 of csrc/common.h on a Python int: the host derives its seeds with the generator the kernels draw from"""
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


def _floats(vals, n):
    """HOST float[n] argument (configuration constants passed by value into a launch)"""
    return (ctypes.c_float * n)(*[float(v) for v in vals])


def _workspace256(nbytes, device):
    """-> (uint8 tensor that owns the memory, pointer to `nbytes` bytes inside it on a 256-byte boundary)"""
    ws = torch.empty(nbytes + 256, device=device, dtype=torch.uint8)
    return ws, ctypes.c_void_p((ws.data_ptr() + 255) // 256 * 256)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """the current stream's hipStream_t (the raw-handle query: ~0.3 us; building a torch.cuda.Stream object per launch cost
    10 us x ~55 launches per step of host time)"""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dt(t_or_dtype):
    d = t_or_dtype if isinstance(t_or_dtype, torch.dtype) else t_or_dtype.dtype
    if d == torch.float32:
        return SW_F32
    if d == torch.bfloat16:
        return SW_BF16
    raise TypeError(f"unsupported dtype {d}")


class KernelTimer:
    """Optional in-process timing of tagged launches with HIP events recorded on the launch stream (used by
    bench.py to price the dominant kernels live; off by default => zero overhead)."""

    def __init__(self, tags, family=None):
        """family: optional callable tag -> one of `tags` (or None): several call sites timed under one key, e.g. every backbone
        convolution's forward launch (tags "plain3.conv2_fwd", ...) as "conv_fwd" """
        self.tags = set(tags)
        self.family = family
        self.pairs = {t: [] for t in tags}
        self.work = {t: 0.0 for t in tags}        # algorithmic work (FLOP or bytes) noted by the call sites of a tag

    def _key(self, tag):
        if tag in self.tags:
            return tag
        return self.family(tag) if self.family is not None else None

    def note(self, tag, amount):
        tag = self._key(tag)
        if tag is not None:
            self.work[tag] += float(amount)

    def wrap(self, tag, fn):
        tag = self._key(tag)
        if tag is None:
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        self.pairs[tag].append((a, b))
        return r

    def summary_ms(self):
        torch.cuda.synchronize()
        return {t: [a.elapsed_time(b) for a, b in ps] for t, ps in self.pairs.items()}


TIMER = None


_WORKER_STREAMS = {}
_WORKER_ROLES = ("main", "side", "upd", "chk")


def worker_stream(role, device=None):
    """The process's ONE stream per role and device — "main" (a step graph's capture / replay stream), "side" (the second backbone
    scale, the Stage-3 teacher), "upd" (the data-parallel bucket updates), "chk" (the speculation ledger's comparison).  All four are
    created together, in this order, the first time any is asked for.  Why not a fresh torch.cuda.Stream() per model / trainer: the
    runtime spreads streams over a handful of hardware queues in creation order, and two streams that are meant to run side by side
    but landed on one queue serialise — or stall each other at their event waits.  With every trainer of a process creating its own
    streams, the SAME code measured 12.8 or 18.9 ms per Stage-3 iteration and 8.5 or 11.3 ms per data-parallel step depending on how
    many models had lived in the process before (bench.py's extras).  Sharing a role's stream between models only adds ordering."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    got = _WORKER_STREAMS.get(idx)
    if got is None:
        got = _WORKER_STREAMS[idx] = {r: torch.cuda.Stream(device=torch.device("cuda", idx)) for r in _WORKER_ROLES}
    return got[role]


class capture_guard:
    """Around a hipGraph capture: Python's cycle collector stays off.  A collection that happens to run inside the capture — it can,
    on the autograd thread too, whenever the allocation counter says so — may finalize an older torch.cuda.CUDAGraph that was
    waiting in a reference cycle (a deleted Trainer and its graphs), and destroying a graph while ANY stream of the process
    captures is an error of the runtime ("operation not permitted when stream is capturing" from ~CUDAGraph: the whole process
    dies; seen in bench.py between two of its short runs).  Collect first, then disable until the capture is over."""

    def __enter__(self):
        import gc
        gc.collect()
        self._was = gc.isenabled()
        gc.disable()
        return self

    def __exit__(self, *exc):
        import gc
        if self._was:
            gc.enable()
        return False


def grad_target(param, shape, dev):
    """Where a weight-gradient GEMM writes.  Under DistributedDataParallel(gradient_as_bucket_view=True) the Trainer remembers the
    bucket view each parameter's gradient lived in last step (`param._sw_grad_view`); writing the new gradient THERE lets the
    reducer find `grad.is_alias_of(bucket_view)` and skip its copy of the tensor into the bucket (fc6: 411 MB read + written per
    step).  Only when the parameter holds no gradient (no accumulation in flight) and the view still fits; else a fresh tensor."""
    view = param.__dict__.get("_sw_grad_view")
    if (view is not None and param.grad is None and tuple(view.shape) == tuple(shape) and view.device == dev
            and view.dtype == torch.float32 and view.is_contiguous()):
        return view.detach()          # a tensor object of its own on the bucket's storage: autograd adopts a gradient only if nobody else holds it
    return torch.empty(*shape, device=dev, dtype=torch.float32)


def _launch(tag, fn):
    if TIMER is None or tag is None:
        return fn()
    return TIMER.wrap(tag, fn)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("sos-wsod_amd kernels need GPU tensors (there is no CPU fallback)")


def make_epilogue(bias=None, relu=False, drop_mask=None, drop_scale=2.0, relu_ref=None, ref_scale=1.0,
                  out_dtype=torch.float32, atomic=False, absmax_out=None, drop_hash=None, splitk_workspace=None, residual=None,
                  row_scale=None):
    """drop_hash=(seed, offset, p[, device counter]): dropout decided in the epilogue by the hash that sw_dropout_mask uses (no
    mask tensor); with a device counter (uint64 scalar tensor) the stream position is offset + *counter at run time"""
    ep = Epilogue()
    ep.bias = None if bias is None else bias.data_ptr()
    ep.relu = int(relu)
    ep.drop_mask = None if drop_mask is None else drop_mask.data_ptr()
    ep.ld_drop = 0 if drop_mask is None else drop_mask.stride(0)
    ep.drop_scale = float(drop_scale)
    if relu_ref is not None and relu_ref.dim() != 2:
        raise ValueError("relu_ref: a (rows, columns) matrix (its row pitch is the reference's leading dimension)")
    ep.relu_ref = None if relu_ref is None else relu_ref.data_ptr()
    ep.ld_ref = 0 if relu_ref is None else relu_ref.stride(0)
    ep.ref_scale = float(ref_scale)
    ep.ref_dtype = SW_F32 if relu_ref is None else dt(relu_ref)
    ep.out_dtype = dt(out_dtype)
    ep.accumulate_atomic = int(atomic)
    ep.absmax_out = None if absmax_out is None else absmax_out.data_ptr()
    ep.splitk_workspace = None if splitk_workspace is None else splitk_workspace.data_ptr()
    if drop_hash is not None and drop_mask is None:
        ep.drop_seed, ep.drop_offset, ep.drop_hash_p = int(drop_hash[0]) & (2 ** 64 - 1), int(drop_hash[1]), float(drop_hash[2])
        if len(drop_hash) > 3 and drop_hash[3] is not None:
            ep.drop_offset_dev = drop_hash[3].data_ptr()
    if residual is not None and residual.dim() != 2:
        raise ValueError("residual: a (rows, columns) matrix")
    ep.residual = None if residual is None else residual.data_ptr()
    ep.ld_res = 0 if residual is None else residual.stride(0)
    ep.res_dtype = SW_F32 if residual is None else dt(residual)
    ep.fold_row_scale = None if row_scale is None else row_scale.data_ptr()        # plain f32-output GEMMs: C[m][:] *= row_scale[m]
    ep._keepalive = (bias, drop_mask, relu_ref, absmax_out, splitk_workspace, drop_hash, residual, row_scale)     # the struct holds raw pointers only
    return ep


def gemm(A, B, C, M, N, K, a_kstrided=False, b_kstrided=False, lda=None, ldb=None, ldc=None, ep=None, splitk=1, tag=None):
    """C[m][n] = sum_k A(m,k) B(k,n); see sw_gemm.  A and B share one dtype (f32 / bf16)."""
    _need_gpu(A, B, C)
    lda = A.stride(0) if lda is None else lda
    ldb = B.stride(0) if ldb is None else ldb
    ldc = C.stride(0) if ldc is None else ldc
    if ep is None:
        ep = make_epilogue(out_dtype=C.dtype)
    if (C.dtype == torch.float32 or splitk > 1) and not ep.accumulate_atomic and not ep.splitk_workspace:
        # split-K (explicit, or the tail peel of the large weight-gradient GEMMs) through slabs + an ordered fold: no atomics,
        # bitwise reproducible; with an epilogue (bias / residual / ReLU / mask, bf16 C) the fold applies it
        need = int(lib.sw_gemm_splitk_workspace_floats(M, N, K, splitk))
        if need > 0:
            ws = torch.empty(need, device=C.device, dtype=torch.float32)
            ep.splitk_workspace = ws.data_ptr()
            ep._keepalive = ep._keepalive + (ws,)
    check(_launch(tag, lambda: lib.sw_gemm(dt(A), int(a_kstrided), int(b_kstrided), M, N, K, _p(A), lda, _p(B), ldb, _p(C),
                                           ldc, ctypes.byref(ep), splitk, _stream())), "sw_gemm")
    return C


def conv3x3(x, wk, out, dilation, ep, tag=None):
    """x [n][H][W][Cin], wk [Cout][9][Cin], out [n][H][W][Cout]"""
    _need_gpu(x, wk, out)
    n, H, W, Cin = x.shape
    Cout = out.shape[3]
    if TIMER is not None and tag is not None:
        TIMER.note(tag, 2.0 * n * H * W * Cout * 9 * Cin)
    check(_launch(tag, lambda: lib.sw_conv3x3_igemm(dt(x), n, H, W, Cin, Cout, dilation, _p(x), _p(wk), _p(out),
                                                    ctypes.byref(ep), _stream())), "sw_conv3x3_igemm")
    return out


def conv3x3_relu_pool2(x, wk, bias, out_pooled, tag=None):
    """x [n][H][W][Cin] -> out_pooled [n][(H-2)//2+1][(W-2)//2+1][Cout] = maxpool2x2/2(relu(conv3x3(x) + bias)) in one launch
    (sw_conv3x3_relu_pool2); False when the shape is not covered (the caller then runs conv3x3 + maxpool_fwd)"""
    _need_gpu(x, wk, out_pooled)
    n, H, W, Cin = x.shape
    Cout = out_pooled.shape[3]
    if TIMER is not None and tag is not None:
        TIMER.note(tag, 2.0 * n * H * W * Cout * 9 * Cin)
    rc = _launch(tag, lambda: lib.sw_conv3x3_relu_pool2(dt(x), n, H, W, Cin, Cout, _p(x), _p(wk), _p(bias), _p(out_pooled), _stream()))
    if rc < 0:
        check(rc, "sw_conv3x3_relu_pool2")
    return rc == 1


def conv3x3_multi(problems):
    """problems: list of (x NHWC, wk [Cout][9][Cin], out NHWC, epilogue) — stride-1, dilation-1 convolutions of different maps (the FPN
    levels of a detector) in ONE launch of the direct kernel (sw_conv3x3_multi); shapes it does not cover run one by one"""
    from ._lib import ConvProblem
    n = len(problems)
    if n == 0:
        return
    if 1 < n <= 8 and problems[0][0].dtype == torch.bfloat16:
        arr = (ConvProblem * n)()
        for i, (x, wk, out, ep) in enumerate(problems):
            _need_gpu(x, wk, out)
            q = arr[i]
            q.nimg, q.H, q.W, q.Cin = x.shape
            q.Cout = out.shape[3]
            q.in_, q.wk, q.out, q.ep = x.data_ptr(), wk.data_ptr(), out.data_ptr(), ctypes.pointer(ep)
        rc = int(lib.sw_conv3x3_multi(SW_BF16, n, arr, _stream()))
        if rc == 1:
            return
        if rc < 0:
            check(rc, "sw_conv3x3_multi")
    for x, wk, out, ep in problems:
        conv3x3(x, wk, out, 1, ep)


def conv3x3_wgrad(x, dy, dw_oihw, dilation, splitk=1, workspace=None, tag=None, cout_scale=None, accumulate=False):
    """dw_oihw (Cout, Cin, 3, 3) f32 is overwritten (accumulate: added to); workspace: Cout*9*Cin floats (allocated here if None);
    cout_scale (Cout,) f32: dw[co] *= cout_scale[co] inside the slab fold (FrozenBN fold of the gradient)"""
    _need_gpu(x, dy, dw_oihw)
    n, H, W, Cin = x.shape
    Cout = dy.shape[3]
    need = int(lib.sw_conv3x3_wgrad_workspace_floats(dt(x), n, H, W, Cin, Cout, splitk))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=x.device, dtype=torch.float32)
    check(_launch(tag, lambda: lib.sw_conv3x3_wgrad(dt(x), n, H, W, Cin, Cout, dilation, _p(x), _p(dy), _p(dw_oihw),
                                                    _p(workspace), splitk, _p(cout_scale), int(accumulate), _stream())), "sw_conv3x3_wgrad")
    return dw_oihw


def conv3x3_wgrad_small(x, dy, dw_oihw, cout_scale=None, accumulate=False):
    """3x3 weight gradient of a map of a few pixels (sw_conv3x3_wgrad_small): x (n, H, W, Cin), dy (n, H, W, Cout) -> dw (Cout, Cin, 3, 3) f32
    (accumulate: added to dw)"""
    _need_gpu(x, dy, dw_oihw)
    n, H, W, Cin = x.shape
    check(lib.sw_conv3x3_wgrad_small(dt(x), n, H, W, Cin, dy.shape[3], _p(x), _p(dy), _p(cout_scale), _p(dw_oihw), int(accumulate),
                                     _stream()), "sw_conv3x3_wgrad_small")
    return dw_oihw


def conv3x3_wgrad_nslab(x, cout, splitk):
    """slabs that a weight-gradient problem (x, dy -> cout channels, splitk) of conv3x3_wgrad_grouped writes"""
    n, H, W, Cin = x.shape
    return int(lib.sw_conv3x3_wgrad_workspace_floats(dt(x), n, H, W, Cin, cout, splitk)) // (cout * 9 * Cin)


def conv3x3_wgrad_nslab_shape(dtype, n, H, W, Cin, cout, splitk):
    """conv3x3_wgrad_nslab for a batch given by its shape and torch dtype"""
    code = SW_BF16 if dtype == torch.bfloat16 else SW_F32
    return int(lib.sw_conv3x3_wgrad_workspace_floats(code, n, H, W, Cin, cout, splitk)) // (cout * 9 * Cin)


def conv3x3_wgrad_grouped(problems, tag=None):
    """problems: list of (x NHWC, dy NHWC, slabs f32 tensor, dilation, nsplit) — every weight gradient of a backward pass in one
    launch (sw_conv3x3_wgrad_grouped); each writes conv3x3_wgrad_nslab(x, cout, nsplit) slabs at `slabs`"""
    from ._lib import WgradProblem
    n = len(problems)
    if n == 0:
        return
    arr = (WgradProblem * n)()
    for i, (x, dy, slabs, dil, nsplit) in enumerate(problems):
        _need_gpu(x, dy, slabs)
        q = arr[i]
        q.nimg, q.H, q.W, q.Cin = x.shape
        q.Cout, q.dilation, q.nsplit = dy.shape[3], int(dil), int(nsplit)
        q.x, q.dy, q.slabs = x.data_ptr(), dy.data_ptr(), slabs.data_ptr()
    if TIMER is not None and tag is not None:
        TIMER.note(tag, sum(2.0 * x.numel() * 9 * dy.shape[3] for x, dy, _, _, _ in problems))
    check(_launch(tag, lambda: lib.sw_conv3x3_wgrad_grouped(dt(problems[0][0]), n, arr, _stream())), "sw_conv3x3_wgrad_grouped")


def conv3x3_wgrad_fold(workspace, nslab, dw_oihw, cout_scale=None, accumulate=False):
    """dw_oihw (Cout, Cin, 3, 3) f32 = (+=, accumulate) cout_scale[co] * ordered sum of `nslab` consecutive [co][tap][ci] slabs"""
    Cout, Cin = dw_oihw.shape[:2]
    check(lib.sw_conv3x3_wgrad_fold(Cin, Cout, nslab, _p(workspace), _p(dw_oihw), _p(cout_scale), int(accumulate), _stream()),
          "sw_conv3x3_wgrad_fold")
    return dw_oihw


def conv3x3_wgrad_fold_multi(folds):
    """folds: list of (workspace, nslab, dw_oihw): every weight-gradient fold of a backward pass in one launch"""
    from ._lib import WgradFold
    n = len(folds)
    if n == 0:
        return
    arr = (WgradFold * n)()
    for i, (ws, nslab, dw) in enumerate(folds):
        arr[i].Cout, arr[i].Cin, arr[i].nslab = dw.shape[0], dw.shape[1], int(nslab)
        arr[i].workspace, arr[i].dw_oihw = ws.data_ptr(), dw.data_ptr()
    check(lib.sw_conv3x3_wgrad_fold_multi(n, arr, _stream()), "sw_conv3x3_wgrad_fold_multi")


def gemm_kk_nslab(dtype, K, nsplit):
    """slabs a problem of gemm_kk_grouped with this K and split count writes"""
    return int(lib.sw_gemm_kk_grouped_slabs(dt(dtype), int(K), int(nsplit)))


def gemm_kk_grouped(problems):
    """problems: list of (A (K, M) rows of pitch lda, B (K, N) rows of pitch ldb, slabs f32, nsplit): slabs[z] = A_z^T B_z for all of them
    in ONE launch (sw_gemm_kk_grouped: resident 256x256-tile grid over every problem's K-splits)"""
    from ._lib import GemmKKProblem
    n = len(problems)
    if n == 0:
        return
    arr = (GemmKKProblem * n)()
    for i, (A, B, slabs, nsplit) in enumerate(problems):
        _need_gpu(A, B, slabs)
        q = arr[i]
        q.A, q.B, q.slabs = A.data_ptr(), B.data_ptr(), slabs.data_ptr()
        q.K, q.M, q.N, q.nsplit = A.shape[0], A.shape[1], B.shape[1], int(nsplit)
        q.lda, q.ldb = A.stride(0), B.stride(0)
    check(lib.sw_gemm_kk_grouped(dt(problems[0][0]), n, arr, _stream()), "sw_gemm_kk_grouped")


def splitk_fold_multi(folds):
    """folds: list of (workspace, nslab, C (M, N) f32, row_scale or None, accumulate): C = [C +] row_scale[:, None] * sum of the slabs,
    all in ONE launch (sw_splitk_fold_multi)"""
    from ._lib import SplitkFold
    n = len(folds)
    if n == 0:
        return
    arr = (SplitkFold * n)()
    for i, (ws, nslab, C, rs, acc) in enumerate(folds):
        _need_gpu(ws, C)
        q = arr[i]
        q.M, q.N, q.nslab, q.accumulate = C.shape[0], C.shape[1], int(nslab), int(bool(acc))
        q.workspace, q.C, q.ldc, q.row_scale = ws.data_ptr(), C.data_ptr(), C.stride(0), (None if rs is None else rs.data_ptr())
    check(lib.sw_splitk_fold_multi(n, arr, _stream()), "sw_splitk_fold_multi")


def colsum_fold_multi(folds):
    """folds: list of (workspace, n_rows, out): every bias-gradient fold of a backward pass in one launch"""
    from ._lib import ColsumFold
    n = len(folds)
    if n == 0:
        return
    arr = (ColsumFold * n)()
    for i, (ws, rows, out) in enumerate(folds):
        arr[i].N, arr[i].n_partial_rows, arr[i].workspace, arr[i].out = out.numel(), int(rows), ws.data_ptr(), out.data_ptr()
    check(lib.sw_colsum_fold_multi(n, arr, _stream()), "sw_colsum_fold_multi")


def colsum_nrows(X_dtype, M, N):
    """partial rows that a colsum_partial_multi problem writes for an M x N matrix"""
    return int(lib.sw_colsum_workspace_floats(dt(X_dtype), M, N)) // N


def colsum_partial_multi(parts):
    """parts: list of (X 2-D view (M, N) with unit inner stride, workspace f32) — the partial rows of every bias gradient of a backward pass in ONE launch"""
    from ._lib import ColsumPart
    n = len(parts)
    if n == 0:
        return
    arr = (ColsumPart * n)()
    for i, (X, ws) in enumerate(parts):
        _need_gpu(X, ws)
        q = arr[i]
        q.M, q.N = X.shape
        q.X, q.ld, q.workspace = X.data_ptr(), X.stride(0), ws.data_ptr()
    check(lib.sw_colsum_partial_multi(dt(parts[0][0]), n, arr, _stream()), "sw_colsum_partial_multi")


def conv_weight_prep(w_oihw, wk, mode, cin_pad=None):
    Cout, Cin = w_oihw.shape[:2]
    cin_pad = Cin if cin_pad is None else cin_pad
    check(lib.sw_conv_weight_prep(dt(wk), mode, Cout, Cin, cin_pad, _p(w_oihw), _p(wk), _stream()), "sw_conv_weight_prep")
    return wk


def maxpool_fwd(x, out, stride):
    n, H, W, C = x.shape
    check(lib.sw_maxpool2x2_fwd(dt(x), n, H, W, C, stride, _p(x), _p(out), _stream()), "sw_maxpool2x2_fwd")
    return out


def maxpool_bwd(x, dout, din, stride, relu_mask):
    n, H, W, C = x.shape
    check(lib.sw_maxpool2x2_bwd(dt(x), n, H, W, C, stride, _p(x), _p(dout), _p(din), int(relu_mask), _stream()),
          "sw_maxpool2x2_bwd")
    return din


def preprocess(img_u8_chw, out_hwc, mean, std):
    _need_gpu(img_u8_chw, out_hwc)
    H, W, cpad = out_hwc.shape
    m, s = _floats(mean, 3), _floats(std, 3)
    check(lib.sw_preprocess(dt(out_hwc), H, W, cpad, _p(img_u8_chw), m, s, _p(out_hwc), _stream()), "sw_preprocess")
    return out_hwc


def preprocess_multi(imgs_u8_chw, out_nhwc, mean, std):
    """n u8 CHW images of one size -> out [n][H][W][cpad], one launch"""
    _need_gpu(out_nhwc, *imgs_u8_chw)
    n, H, W, cpad = out_nhwc.shape
    assert len(imgs_u8_chw) == n and all(im.is_contiguous() and tuple(im.shape) == (3, H, W) for im in imgs_u8_chw)
    ptrs = (ctypes.c_void_p * n)(*[im.data_ptr() for im in imgs_u8_chw])
    m, s = _floats(mean, 3), _floats(std, 3)
    check(lib.sw_preprocess_multi(dt(out_nhwc), n, H, W, cpad, ptrs, m, s, _p(out_nhwc), _stream()), "sw_preprocess_multi")
    return out_nhwc


def roi_pool_fwd_workspace(n, R, PH, PW, device):
    """scratch for roi_pool_fwd's prepared-task form; uint8, 256-byte aligned by the allocator"""
    return torch.empty(max(16, lib.sw_roi_pool_fwd_workspace_bytes(n, R, PH, PW)), device=device, dtype=torch.uint8)


def roi_pool_fwd(feat, rois, out, argmax, spatial_scale, PH, PW, row_scale=None, row_scale_add=0.0, tag=None, workspace="auto"):
    """feat [n][H][W][C], rois [R][5] f32, out [R][C*PH*PW]; argmax same shape, int32 (h*W+w or -1) or int16/uint16
    storage holding uint16 (h*W+w or 0xFFFF; see argmax_to_int32).  workspace: roi_pool_fwd_workspace(...) tensor, "auto" = allocate
    one here (caching allocator: graph-safe), None = the forms without prepared tasks"""
    _need_gpu(feat, rois, out, argmax)
    n, H, W, C = feat.shape
    R = rois.shape[0]
    if isinstance(workspace, str):
        workspace = roi_pool_fwd_workspace(n, R, PH, PW, feat.device) if R > 0 else None
    check(_launch(tag, lambda: lib.sw_roi_pool_fwd(dt(feat), n, H, W, C, PH, PW, float(spatial_scale), _p(feat), _p(rois), R,
                                                   _p(row_scale), float(row_scale_add), _p(out), _p(argmax), _argmax_bits(argmax),
                                                   _roi_pitch(out, argmax), _p(workspace),
                                                   0 if workspace is None else workspace.numel(), _stream())), "sw_roi_pool_fwd")
    return out, argmax


def _roi_pitch(vals, argmax):
    if vals.stride(0) != argmax.stride(0) or vals.stride(-1) != 1 or argmax.stride(-1) != 1:
        raise ValueError("ROIPool values and argmax must share one row pitch (unit inner stride)")
    return vals.stride(0)


def _argmax_bits(argmax):
    if argmax.dtype == torch.int32:
        return 32
    if argmax.dtype in (torch.int16, torch.uint16):
        return 16
    raise TypeError(f"ROIPool argmax must be int32 or (u)int16, got {argmax.dtype}")


def roi_argmax_dtype(H, W):
    """compact index type for an H x W map: uint16 (int16 storage) below 65535 pixels, else int32"""
    return torch.int16 if H * W < 65535 else torch.int32


def argmax_to_int32(argmax):
    """decode either storage to the reference's int32 convention (-1 = empty bin)"""
    if argmax.dtype == torch.int32:
        return argmax
    a = argmax.view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(a == 0xFFFF, torch.full_like(a, -1), a)


def absmax(x, out=None):
    if out is None:
        out = torch.empty(1, device=x.device, dtype=torch.float32)
    check(lib.sw_absmax(dt(x), x.numel(), _p(x), _p(out), _stream()), "sw_absmax")
    return out


def roi_pool_bwd(dout, argmax, rois, dfeat, PH, PW, row_scale=None, row_scale_add=0.0, relu_ref=None, dout_absmax="auto",
                 tag=None, spatial_scale=0.0):
    """dout_absmax: device scalar >= max|dout| (selects the fixed-point accumulation), "auto" = compute it here,
    None = LDS float atomics.  spatial_scale: the forward's scale (lets large maps skip ROIs outside a workgroup's pixel range)."""
    _need_gpu(dout, argmax, rois, dfeat)
    n, H, W, C = dfeat.shape
    R = rois.shape[0]
    if isinstance(dout_absmax, str):
        dout_absmax = absmax(dout)
    check(_launch(tag, lambda: lib.sw_roi_pool_bwd(dt(dfeat), n, H, W, C, PH, PW, _p(dout), _p(argmax), _argmax_bits(argmax),
                                                   _roi_pitch(dout, argmax), _p(rois), R, _p(row_scale), float(row_scale_add),
                                                   _p(relu_ref), _p(dout_absmax), _p(dfeat), float(spatial_scale), _stream())),
          "sw_roi_pool_bwd")
    return dfeat


def wsddn_mil(logits, V, R, K, cls_col, det_col, gt_onehot, scores, loss_view, dlogits=None, grad_scale=None,
              mean_scores=None, workspace=None):
    """mean_scores: optional [R][>=K] f32 (row pitch = its stride) receiving the view-mean scores"""
    _need_gpu(logits, gt_onehot, scores, loss_view)
    if workspace is None:
        workspace = torch.empty(int(lib.sw_wsddn_workspace_floats(V, R, K)), device=logits.device, dtype=torch.float32)
    check(lib.sw_wsddn_mil(V, R, K, _p(logits), logits.stride(0), cls_col, det_col, _p(gt_onehot), _p(scores),
                           _p(loss_view), _p(dlogits), 0 if dlogits is None else dlogits.stride(0), _p(grad_scale),
                           _p(mean_scores), 0 if mean_scores is None else mean_scores.stride(-2), _p(workspace),
                           _stream()), "sw_wsddn_mil")


def sgd_multi(entries, momentum, grad_scale=1.0):
    """entries: list of dict(param, grad, buf, lr, weight_decay, first, staging=None|staging.entry_of(param), hyper=None|device tensor
    {lr, weight_decay} read by the kernel instead of the two floats).  One launch per 24."""
    from ._lib import SgdTensor
    n = len(entries)
    if n == 0:
        return
    arr = (SgdTensor * n)()
    for i, e in enumerate(entries):
        _fill_sgd_tensor(arr[i], e)
    check(lib.sw_sgd_multi(n, arr, float(momentum), float(grad_scale), _stream()), "sw_sgd_multi")


def _fill_sgd_tensor(d, e):
    p = e["param"]
    g = e.get("grad")
    d.param, d.grad, d.momentum_buf, d.n = p.data_ptr(), (None if g is None else g.data_ptr()), e["buf"].data_ptr(), p.numel()
    d.lr, d.weight_decay, d.first_step = float(e["lr"]), float(e["weight_decay"]), int(e["first"])
    hy = e.get("hyper")
    d.hyper_dev = None if hy is None else hy.data_ptr()
    st = e.get("staging")
    if st is None:
        d.stage_kind = 0
    else:
        d.stage_kind, d.stage_dtype = st["kind"], dt(st["dtype"])
        d.stage0 = None if st["stage0"] is None else st["stage0"].data_ptr()
        d.stage1 = None if st["stage1"] is None else st["stage1"].data_ptr()
        d.d0, d.d1, d.d2, d.ld0, d.ld1 = st["d0"], st["d1"], st["d2"], st["ld0"], st.get("ld1", 0)


def gemm_sgd_fused_supported(dtype, M, N, K, a_kstrided=False, b_kstrided=False):
    """can sw_gemm take an epilogue with `sgd_fused` for this shape (the ping-pong 256x256 form; see sw_epilogue.sgd_fused)?"""
    return bool(lib.sw_gemm_sgd_fused_supported(dt(dtype), int(a_kstrided), int(b_kstrided), int(M), int(N), int(K)))


def attach_sgd_fused(ep, entry, momentum, grad_scale=1.0):
    """ep: an Epilogue for the weight-gradient GEMM of a 2D parameter; entry: the optimizer's record for that parameter (as for sgd_multi,
    without a gradient).  The GEMM then applies the SGD update in its epilogue instead of writing the gradient (sw_epilogue.sgd_fused)."""
    from ._lib import SgdTensor
    d = SgdTensor()
    _fill_sgd_tensor(d, entry)
    ep.sgd_fused = ctypes.addressof(d)
    ep.sgd_momentum, ep.sgd_grad_scale = float(momentum), float(grad_scale)
    ep._keepalive = ep._keepalive + (d, entry["param"], entry["buf"], entry.get("hyper"))
    return ep


def mean_views(x, out):
    V = x.shape[0]
    check(lib.sw_mean_views(V, out.numel(), _p(x), _p(out), _stream()), "sw_mean_views")
    return out


def oicr_mean_probs(logits, V, R, K, n_rounds, cls_col0, col_stride, out):
    """out [n_rounds][R][K+1] = view-mean softmax of each refinement head's class logits"""
    _need_gpu(logits, out)
    check(lib.sw_oicr_mean_probs(V, R, K, n_rounds, _p(logits), logits.stride(0), cls_col0, col_stride, _p(out), _stream()),
          "sw_oicr_mean_probs")
    return out


def mine_workspace_bytes(R, top_k, G, n_rounds=1):
    return int(lib.sw_mine_workspace_bytes(R, top_k, G)) * n_rounds


def oicr_mine_label(scores, gt_classes_i32, boxes, K, top_k, thresh, nms_thresh, iou_bg, iou_fg, lab_class, lab_weight,
                    lab_index, pgt_count, pgt_index, pgt_class, pgt_score, workspace, *, cand_boxes=None, cand_from=0,
                    seed_rule=0, lab_box=None, pgt_box=None):
    """scores [R][ncol] (one round) or [n_rounds][R][ncol]; the outputs carry the same leading dimension.
    cand_boxes [n_rounds - cand_from][R][G][4]: class-specific candidate boxes of the rounds >= cand_from (OICRPLUS.BBOX_UPDATE);
    seed_rule 1: one seed per class in class order, no threshold, no NMS (WSL.REFINE_MIST False; top_k must be 1);
    lab_box [n_rounds][R][4] / pgt_box [n_rounds][top_k*G][4]: the matched pseudo box of every proposal / the kept list's boxes"""
    _need_gpu(scores, gt_classes_i32, boxes)
    n_rounds = 1 if scores.dim() == 2 else scores.shape[0]
    R, ncol = scores.shape[-2:]
    G = gt_classes_i32.numel()
    if cand_boxes is not None:
        assert cand_boxes.dtype == torch.float32 and cand_boxes.is_contiguous() and \
            cand_boxes.numel() == (n_rounds - cand_from) * R * G * 4, "cand_boxes is [n_rounds - cand_from][R][G][4] f32"
    for t, rows in ((lab_box, R), (pgt_box, int(top_k) * G)):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n_rounds * rows * 4)
    _launch("mine_label", lambda: check(
        lib.sw_oicr_mine_label(R, ncol, K, n_rounds, _p(scores), _p(gt_classes_i32), G, _p(boxes), int(top_k),
                               float(thresh), float(nms_thresh), float(iou_bg), float(iou_fg), _p(lab_class),
                               _p(lab_weight), _p(lab_index), _p(pgt_count), _p(pgt_index), _p(pgt_class), _p(pgt_score),
                               _p(workspace), _p(cand_boxes), int(cand_from), int(seed_rule), _p(lab_box), _p(pgt_box),
                               _stream()), "sw_oicr_mine_label"))


def oicr_update_boxes(logits, V, R, K, n_heads, box_col, col_stride, boxes, gt_classes_i32, dx_sign, reg_weights, scale_clamp, out):
    """out [n_heads][R][G][4] = apply_deltas(view-mean signed deltas of refinement head k, class gt_classes[g]; boxes [R][4] of view 0):
    the next round's class-specific candidate boxes (OICRPLUS.BBOX_UPDATE).  dx_sign: device int32[V], -1 for a flipped view"""
    _need_gpu(logits, boxes, gt_classes_i32, dx_sign, out)
    G = gt_classes_i32.numel()
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n_heads * R * G * 4
    assert dx_sign.dtype == torch.int32 and dx_sign.numel() == V and boxes.is_contiguous()
    assert logits.shape[0] >= V * R and 0 <= box_col and box_col + (n_heads - 1) * col_stride + 4 * K <= logits.shape[1]
    check(lib.sw_oicr_update_boxes(V, R, K, G, n_heads, _p(logits), logits.stride(0), box_col, col_stride, _p(boxes),
                                   _p(gt_classes_i32), _p(dx_sign), _floats(reg_weights, 4), float(scale_clamp), _p(out),
                                   _stream()), "sw_oicr_update_boxes")
    return out


def oicr_refine_loss(logits, V, R, K, cls_col, box_col, boxes, lab_class, lab_weight, lab_index, pred_view, reg_weights,
                     loss_view, dlogits=None, grad_scale=None, workspace=None, n_rounds=1, col_stride=0, tgt_box0=None):
    """n_rounds heads at columns cls_col/box_col + k*col_stride; lab_* [n_rounds][R]; loss_view [n_rounds][2][V];
    grad_scale device float[2*n_rounds]; tgt_box0 [n_rounds][R][4]: view 0's regression target boxes (OICRPLUS.BBOX_UPDATE:
    the matched refined pseudo boxes) instead of boxes[0][lab_index]"""
    rw = _floats(reg_weights, 4)
    if workspace is None:
        workspace = torch.empty(n_rounds * 2 * V * R, device=logits.device, dtype=torch.float32)
    assert tgt_box0 is None or (tgt_box0.dtype == torch.float32 and tgt_box0.is_contiguous() and tgt_box0.numel() == n_rounds * R * 4)
    check(lib.sw_oicr_refine_loss(V, R, K, n_rounds, _p(logits), logits.stride(0), cls_col, box_col, col_stride, _p(boxes),
                                  _p(lab_class), _p(lab_weight), _p(lab_index), _p(pred_view), rw, _p(loss_view),
                                  _p(dlogits), 0 if dlogits is None else dlogits.stride(0), _p(grad_scale), _p(workspace),
                                  _p(tgt_box0), _stream()), "sw_oicr_refine_loss")


def colsum(X, M, N, out, ld=None, accumulate=False):
    """out[n] = sum_m X[m, n] (f32), deterministic: partial rows per row chunk + an ordered fold (no zero fill, no atomics);
    accumulate: out[n] += the sum"""
    need = int(lib.sw_colsum_workspace_floats(dt(X), M, N))
    ws = torch.empty(max(need, 4), device=X.device, dtype=torch.float32)
    check(lib.sw_colsum(dt(X), M, N, _p(X), X.stride(0) if ld is None else ld, _p(out), _p(ws), int(accumulate), _stream()), "sw_colsum")
    return out


def convert_2d(src_f32, dst, rows, cols, ld_src=None, ld_dst=None):
    check(lib.sw_convert_2d(dt(dst), rows, cols, _p(src_f32), src_f32.stride(0) if ld_src is None else ld_src, _p(dst),
                            dst.stride(0) if ld_dst is None else ld_dst, _stream()), "sw_convert_2d")
    return dst


def split_bf16x3(src_f32, side, along_rows=False, out=None):
    """the K-concatenated three-piece bf16 operand of an f32 matrix (sw_split_bf16x3): (rows, cols) f32 -> (rows, 6 cols) bf16, or
    (6 rows, cols) with along_rows.  side 0 = the A operand's block pattern, 1 = the B operand's.  Row pitch padded by 128 elements."""
    _need_gpu(src_f32)
    rows, cols = src_f32.shape
    assert src_f32.dtype == torch.float32 and src_f32.stride(1) == 1
    shape = (6 * rows, cols) if along_rows else (rows, 6 * cols)
    if out is None or tuple(out.shape) != shape:
        out = torch.empty(shape[0], shape[1] + 128, device=src_f32.device, dtype=torch.bfloat16)[:, :shape[1]]
    check(lib.sw_split_bf16x3(rows, cols, _p(src_f32), src_f32.stride(0), _p(out), out.stride(0), int(side), int(bool(along_rows)), _stream()),
          "sw_split_bf16x3")
    return out


def gemm_f32x3(A, B, C, M, N, K, a_kstrided=False, b_kstrided=False, ep=None, tag=None, A3=None, B3=None):
    """C = A . B for f32 operands at (about) f32 accuracy on the bf16 MFMA: both operands split into three bf16 pieces, six products
    accumulated in f32 as ONE bf16 GEMM over 6 K (sw_split_bf16x3).  A3 / B3: an operand already split (weights, cached per update).
    Operand forms as ops.gemm: A (M, K) or, a_kstrided, (K, M); B (N, K) or, b_kstrided, (K, N)."""
    if A3 is None:
        A3 = split_bf16x3(A, 0, along_rows=a_kstrided)
    if B3 is None:
        B3 = split_bf16x3(B, 1, along_rows=b_kstrided)
    return gemm(A3, B3, C, M, N, 6 * K, a_kstrided=a_kstrided, b_kstrided=b_kstrided, ep=ep, tag=tag)


def convert_2d_t(src_f32, dst, rows, cols):
    """dst[c][r] = src[r][c] in dst's dtype (rows, cols multiples of 64)"""
    check(lib.sw_convert_2d_t(dt(dst), rows, cols, _p(src_f32), src_f32.stride(0), _p(dst), dst.stride(0), _stream()),
          "sw_convert_2d_t")
    return dst


def fill_zero(t):
    check(lib.sw_fill_zero(_p(t), t.numel() * t.element_size(), _stream()), "sw_fill_zero")
    return t


def dropout_mask(keep_u8, seed, offset, p=0.5):
    check(lib.sw_dropout_mask(_p(keep_u8), keep_u8.numel(), int(seed) & (2 ** 64 - 1), int(offset), float(p), _stream()),
          "sw_dropout_mask")
    return keep_u8


def sgd_momentum_step(param, grad, buf, lr, momentum, weight_decay, first_step, grad_scale=1.0):
    check(lib.sw_sgd_momentum_step(_p(param), _p(grad), _p(buf), param.numel(), float(lr), float(momentum),
                                   float(weight_decay), int(first_step), float(grad_scale), _stream()),
          "sw_sgd_momentum_step")


def loss_finalize(loss_view, out, total=None):
    """loss_view [n_losses][V] or [n_images][n_losses][V] -> out[n_losses] (mean over views and images), total[1] = sum"""
    if loss_view.dim() == 2:
        loss_view = loss_view[None]
    B, n, V = loss_view.shape
    check(lib.sw_loss_finalize(n, V, B, _p(loss_view), _p(out), _p(total), _stream()), "sw_loss_finalize")
    return out


def scale_cols_loss(src_f32, g_losses, g_total, col_to_loss_i32, mul, dst, M, N, n_valid):
    check(lib.sw_scale_cols_loss(dt(dst), M, N, n_valid, _p(src_f32), src_f32.stride(0), _p(g_losses), _p(g_total),
                                 _p(col_to_loss_i32), float(mul), _p(dst), dst.stride(0), _stream()), "sw_scale_cols_loss")
    return dst


def resize_pass_u8(src, dst, bounds_i32, kk_i32, ksize, horizontal, dst_flip=None):
    """one pass of Pillow's 8-bit resize (sw_resize_pass_u8): src (C,H,W) u8 -> dst (C,H,out) / (C,out,W).  `src` may be a
    window of a larger planar image (unit pixel stride, the parent's row / plane strides): a crop costs no copy"""
    _need_gpu(src, dst, bounds_i32, kk_i32)
    C, H, W = src.shape
    assert src.stride(2) == 1 and dst.is_contiguous() and (dst_flip is None or dst_flip.is_contiguous())
    out_size = dst.shape[2] if horizontal else dst.shape[1]
    check(lib.sw_resize_pass_u8(C, H, W, src.stride(1), src.stride(0), out_size, int(horizontal), _p(src), _p(bounds_i32),
                                _p(kk_i32), int(ksize), _p(dst), _p(dst_flip), _stream()), "sw_resize_pass_u8")
    return dst


def color_jitter_u8(src, w_bright=None, w_sat=None, with_flip=False):
    """RandomBrightness / RandomSaturation blends on a planar (3,H,W) u8 image (sw_color_jitter_u8); weights None = that blend
    is skipped.  -> out, or (out, x-mirrored out)"""
    import numpy as np
    _need_gpu(src)
    assert src.dtype == torch.uint8 and src.dim() == 3 and src.shape[0] == 3 and src.is_contiguous()
    out = torch.empty_like(src)
    flip = torch.empty_like(src) if with_flip else None
    mode = (1 if w_bright is not None else 0) | (2 if w_sat is not None else 0)
    wb = float(np.float32(w_bright)) if w_bright is not None else 1.0        # numpy scales the float32 image by float32(w)
    ws = float(np.float32(w_sat)) if w_sat is not None else 1.0
    src_w = (1 - float(w_sat)) if w_sat is not None else 0.0                   # `1 - w`: a python double in the reference
    check(lib.sw_color_jitter_u8(src.shape[1], src.shape[2], mode, _p(src), wb, src_w, ws, _p(out), _p(flip), _stream()),
          "sw_color_jitter_u8")
    return (out, flip) if with_flip else out


_AUG_OPS = {"brightness": 0, "contrast": 1, "saturation": 2, "hue": 3}


def _fill_aug_recipe(c, recipe):
    """strong_aug.Recipe -> sw_aug_recipe: op names to codes, the hue factor to its H-channel shift (`int(hue * 255)` truncated
    toward zero, modulo 256 — the rule chosen for the reference's `np.uint8(negative float)`), sigma to Pillow's integer box weights"""
    from ._lib import lib as _l
    order = tuple(recipe.order)
    assert len(order) <= 4 and len(set(order)) == len(order) and all(o in _AUG_OPS for o in order), \
        f"order {order!r}: distinct ops out of {tuple(_AUG_OPS)}"
    c.seed, c.key = int(recipe.seed) & 0xFFFFFFFFFFFFFFFF, int(recipe.key) & 0xFFFFFFFFFFFFFFFF
    for s in range(4):
        c.order[s] = _AUG_OPS[order[s]] if s < len(order) else -1
    c.factor[0], c.factor[1], c.factor[2], c.factor[3] = recipe.brightness, recipe.contrast, recipe.saturation, recipe.hue
    if "hue" in order and not -0.5 <= recipe.hue <= 0.5:
        raise ValueError(f"hue factor {recipe.hue} is not in [-0.5, 0.5]")
    c.hue_shift = int(recipe.hue * 255) % 256
    c.grayscale = 1 if recipe.grayscale else 0
    c.blur_r = -1
    if recipe.blur_sigma is not None:
        r, ww, fw = ctypes.c_int32(), ctypes.c_uint32(), ctypes.c_uint32()
        check(_l.sw_gaussian_blur_weights(float(recipe.blur_sigma), ctypes.byref(r), ctypes.byref(ww), ctypes.byref(fw)),
              "sw_gaussian_blur_weights")
        c.blur_r, c.blur_ww, c.blur_fw = r.value, ww.value, fw.value
    rects = tuple(recipe.rects)
    assert len(rects) <= 3
    for e in range(3):
        t, l, h, w = rects[e] if e < len(rects) and rects[e] is not None else (0, 0, 0, 0)
        c.rect[e][0], c.rect[e][1], c.rect[e][2], c.rect[e][3] = int(t), int(l), int(h), int(w)
    return c


def _check_aug_image(img, recipe):
    _need_gpu(img)
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[0] == 3 and img.is_contiguous(), "planar (3, H, W) uint8, contiguous"
    H, W = img.shape[1], img.shape[2]
    for rc in recipe.rects:
        if rc is not None and rc[2] > 0:
            t, l, h, w = rc
            assert 0 <= t and 0 <= l and h > 0 and w > 0 and t + h <= H and l + w <= W, f"rectangle {rc} leaves the {H} x {W} image"
    return H, W


def strong_augment_u8(img, recipe, out=None):
    """The Stage-3 strong augmentation of one planar (3, H, W) u8 image (sw_strong_aug_u8): `recipe` is a strong_aug.Recipe —
    colour jitter in its drawn order, grayscale, Gaussian blur, up to three erased rectangles; pixels equal to Pillow's.
    -> out (a new tensor unless given; never `img` itself)"""
    from ._lib import AugRecipe
    H, W = _check_aug_image(img, recipe)
    if out is None:
        out = torch.empty_like(img)
    _need_gpu(out)
    assert out.shape == img.shape and out.dtype == torch.uint8 and out.is_contiguous() and out.data_ptr() != img.data_ptr()
    ws = torch.empty(lib.sw_strong_aug_workspace_bytes(H, W), dtype=torch.uint8, device=img.device)
    c = _fill_aug_recipe(AugRecipe(), recipe)
    check(lib.sw_strong_aug_u8(H, W, _p(img), ctypes.byref(c), _p(out), _p(ws), _stream()), "sw_strong_aug_u8")
    return out


def strong_augment_multi_u8(imgs, recipes, outs=None):
    """strong_augment_u8 for a list of images of different sizes in one launch sequence (sw_strong_aug_multi_u8): the per-image
    pointers, sizes and recipes travel as one record array (pinned host buffer, asynchronous copy: no host synchronisation).
    Bit-identical to the per-image calls.  -> list of outputs"""
    from ._lib import AugItem
    assert len(imgs) == len(recipes)
    n = len(imgs)
    if n == 0:
        return []
    dev = imgs[0].device
    if outs is None:
        outs = [torch.empty_like(im) for im in imgs]
    sizes = [_check_aug_image(im, rc) for im, rc in zip(imgs, recipes)]
    per = [lib.sw_strong_aug_workspace_bytes(h, w) for h, w in sizes]
    ws = torch.empty(sum(per), dtype=torch.uint8, device=dev)
    stage = torch.empty(n * ctypes.sizeof(AugItem), dtype=torch.uint8, pin_memory=True)
    items = (AugItem * n).from_address(stage.data_ptr())
    stages, off = 0, ws.data_ptr()
    for i, (im, rc, o) in enumerate(zip(imgs, recipes, outs)):
        _need_gpu(o)
        assert im.device == dev and o.shape == im.shape and o.dtype == torch.uint8 and o.is_contiguous() and o.data_ptr() != im.data_ptr()
        it = items[i]
        it.src, it.out, it.tmp, it.lsum = im.data_ptr(), o.data_ptr(), off, off + per[i] - 256
        it.H, it.W = sizes[i]
        _fill_aug_recipe(it.recipe, rc)
        stages |= (2 if it.recipe.blur_r >= 0 else 4) | (1 if "contrast" in rc.order else 0)
        off += per[i]
    items_dev = stage.to(dev, non_blocking=True)
    check(lib.sw_strong_aug_multi_u8(n, _p(items_dev), max(h for h, _ in sizes), max(w for _, w in sizes), stages, _stream()),
          "sw_strong_aug_multi_u8")
    return outs


def transpose_2d(src, dst, rows, cols):
    """dst[c][r] = src[r][c]; src (rows, cols), dst (cols, rows), same dtype, unit inner stride"""
    _need_gpu(src, dst)
    check(lib.sw_transpose_2d(dt(src), rows, cols, _p(src), src.stride(0), _p(dst), dst.stride(0), _stream()), "sw_transpose_2d")
    return dst


class StagePlan:
    """The device-resident entry table of sw_stage_weights_multi for one model and compute dtype: built once (the tensors it points
    at must stay where they are: parameters / buffers are updated in place, the destinations are owned by the plan's entries),
    run() = one launch.  entries: dicts(kind, w, dst, bn=None | (weight, bias, mean, var), scale=None, shift=None)."""

    def __init__(self, entries, compute_dtype, eps=1e-5):
        from ._lib import StageDesc
        n = len(entries)
        arr = (StageDesc * max(n, 1))()
        blocks = 0
        keep = []
        for i, e in enumerate(entries):
            w = e["w"]
            _need_gpu(w, e["dst"])
            if w.dtype != torch.float32 or not w.is_contiguous() or not e["dst"].is_contiguous():
                raise TypeError("stage plan takes contiguous float32 sources and contiguous destinations")
            kind = int(e["kind"])
            rows, cols = (w.shape[0], w.numel() // w.shape[0]) if kind in (0, 3) else (w.shape[0], w.shape[1])
            want = torch.float32 if kind == 3 else compute_dtype
            if e["dst"].dtype != want or e["dst"].numel() < w.numel():
                raise TypeError("stage plan destination has the wrong dtype or size")
            d = arr[i]
            d.w, d.dst, d.kind, d.rows, d.cols, d.block_start = w.data_ptr(), e["dst"].data_ptr(), kind, rows, cols, blocks
            bn = e.get("bn")
            if bn is not None:
                for t in bn:
                    if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != rows:
                        raise TypeError("FrozenBN buffers must be contiguous float32 of Cout elements")
                d.bn_weight, d.bn_bias, d.bn_mean, d.bn_var = (t.data_ptr() for t in bn)
                d.scale = None if e.get("scale") is None else e["scale"].data_ptr()
                d.shift = None if e.get("shift") is None else e["shift"].data_ptr()
            blocks += int(lib.sw_stage_blocks(kind, rows, cols))
            keep.append((w, e["dst"], bn, e.get("scale"), e.get("shift")))
        self.n, self.blocks, self.eps, self.dtype = n, blocks, float(eps), compute_dtype
        self._keep = keep
        self.ptrs = tuple(w.data_ptr() for w, *_ in keep)
        raw = bytes(arr) if n else b""
        self.table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(entries[0]["w"].device) if n else None

    def run(self):
        if self.n:
            check(lib.sw_stage_weights_multi(dt(self.dtype), self.n, self.table.data_ptr(), self.blocks, self.eps, _stream()),
                  "sw_stage_weights_multi")


class EmaPlan:
    """the host-side argument arrays of sw_ema_multi for fixed lists of tensors (built once: ~600 state-dict entries of a detector)"""

    def __init__(self, teacher, student):
        n = len(teacher)
        assert n == len(student)
        for t, s_ in zip(teacher, student):
            _need_gpu(t, s_)
            if t.dtype != torch.float32 or s_.dtype != torch.float32 or not t.is_contiguous() or not s_.is_contiguous() or t.numel() != s_.numel():
                raise TypeError("ema_multi takes matching contiguous float32 tensors")
        self.n = n
        self.tp = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in teacher])
        self.sp = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in student])
        self.ne = (ctypes.c_long * max(n, 1))(*[t.numel() for t in teacher])
        self._keep = (list(teacher), list(student))

    def run(self, keep_rate):
        if self.n:
            check(lib.sw_ema_multi(self.n, self.tp, self.sp, self.ne, float(keep_rate), _stream()), "sw_ema_multi")


def ema_multi(teacher, student, keep_rate):
    """teacher[i] <- student[i] * (1 - keep_rate) + teacher[i] * keep_rate over lists of contiguous f32 tensors (sw_ema_multi)"""
    EmaPlan(teacher, student).run(keep_rate)


def weighted_sum(values, weights, out):
    """out[i] = values[i] * weights[i] (f32 scalars anywhere on the device), out[n] = their sum in index order (sw_weighted_sum)"""
    n = len(values)
    _need_gpu(out, *values)
    assert all(v.dtype == torch.float32 and v.numel() == 1 for v in values) and out.dtype == torch.float32 and out.numel() >= n + 1
    ptrs = (ctypes.c_void_p * n)(*[v.data_ptr() for v in values])
    ws = _floats(weights, n)
    check(lib.sw_weighted_sum(n, ptrs, ws, _p(out), _stream()), "sw_weighted_sum")
    return out


def scale_scalars(g, weights, out):
    """out[i] = g * weights[i] (sw_scale_scalars)"""
    n = len(weights)
    _need_gpu(g, out)
    ws = _floats(weights, n)
    check(lib.sw_scale_scalars(n, _p(g), ws, _p(out), _stream()), "sw_scale_scalars")
    return out


def threshold_select(scores, classes, boxes, thres, allowed=None):
    """-> (count[1] i32, boxes [n,4], classes [n] i32 or None, scores [n], index [n] i32): entries with score > thres (and class in
    `allowed`, an int32 device tensor, when given: an empty one is an empty label set and keeps nothing), compacted in input order;
    the first count rows are valid"""
    _need_gpu(scores, boxes)
    n = scores.shape[0]
    dev = scores.device
    cnt = torch.empty(1, device=dev, dtype=torch.int32)
    ob = torch.empty(max(n, 1), 4, device=dev); osc = torch.empty(max(n, 1), device=dev)
    oc = torch.empty(max(n, 1), device=dev, dtype=torch.int32) if classes is not None else None
    oi = torch.empty(max(n, 1), device=dev, dtype=torch.int32)
    n_allowed = 0 if allowed is None else allowed.numel()
    if allowed is not None and classes is None:
        raise ValueError("threshold_select: a class filter needs the classes")
    # the entry reads NULL as "no filter", and an empty tensor has no address: hand it one it never reads, with n_allowed = 0
    allowed_p = _p(allowed) if n_allowed or allowed is None else _p(cnt)
    check(lib.sw_threshold_select(n, _p(scores), _p(classes), _p(boxes), float(thres), allowed_p, n_allowed, _p(cnt), _p(ob), _p(oc),
                                  _p(osc), _p(oi), _stream()), "sw_threshold_select")
    return cnt, ob, oc, osc, oi


def copy_multi(pairs):
    """[(src, dst)] contiguous device tensors of equal dtype and shape: all copied by one launch"""
    from ._lib import CopyDesc
    pairs = [(s, d) for s, d in pairs if d.numel()]
    if not pairs:
        return
    arr = (CopyDesc * len(pairs))()
    for i, (s, d) in enumerate(pairs):
        assert s.is_cuda and d.is_cuda and s.dtype == d.dtype and s.shape == d.shape and s.is_contiguous() and d.is_contiguous()
        arr[i].src, arr[i].dst, arr[i].bytes = s.data_ptr(), d.data_ptr(), d.numel() * d.element_size()
    check(lib.sw_copy_multi(len(pairs), arr, _stream()), "sw_copy_multi")


def focal_loss(logits, targets_i32, gamma, loss, dlogits=None):
    """loss[0] = sum_r (1 - p_r)^gamma CE_r / N (sw_focal_loss); dlogits (N, C) f32 optional"""
    _need_gpu(logits, targets_i32, loss)
    N, C = logits.shape
    ws = torch.empty(N, device=logits.device, dtype=torch.float32)
    check(lib.sw_focal_loss(N, C, _p(logits), logits.stride(0), _p(targets_i32), float(gamma), _p(loss), _p(dlogits),
                            0 if dlogits is None else dlogits.stride(0), _p(ws), _stream()), "sw_focal_loss")
    return loss


def counter_add(counter_u64, increment):
    """*counter += increment in stream order (the device-resident dropout stream position)"""
    check(lib.sw_counter_add(_p(counter_u64), int(increment), _stream()), "sw_counter_add")


def pack_views(box_list, obj_list, boxes, obj, rois):
    """4 x (R,4) f32 boxes + 4 x (R,) f32 objectness (contiguous device tensors) -> boxes (4,R,4), obj (4,R), rois (2,2R,5)"""
    _need_gpu(*box_list, *obj_list, boxes, obj, rois)
    R = box_list[0].shape[0]
    bp = (ctypes.c_void_p * 4)(*[b.data_ptr() for b in box_list])
    op = (ctypes.c_void_p * 4)(*[o.data_ptr() for o in obj_list])
    check(lib.sw_pack_views(R, bp, op, _p(boxes), _p(obj), _p(rois), _stream()), "sw_pack_views")


def nchw_to_nhwc(x_nchw_f32, out_nhwc):
    N, C, H, W = x_nchw_f32.shape
    check(lib.sw_nchw_to_nhwc(dt(out_nhwc), N, C, H, W, out_nhwc.shape[3], _p(x_nchw_f32), _p(out_nhwc), _stream()),
          "sw_nchw_to_nhwc")
    return out_nhwc


def relu_bwd(ref, grad, out=None):
    """out = ref > 0 ? grad : 0; in place on `grad` when no `out` is given"""
    out = grad if out is None else out
    check(lib.sw_relu_bwd(dt(grad), grad.numel(), _p(ref), _p(grad), _p(out), _stream()), "sw_relu_bwd")
    return out


def scale_cols(src_f32, colscale, dst, M, N):
    check(lib.sw_scale_cols(dt(dst), M, N, _p(src_f32), src_f32.stride(0), _p(colscale), _p(dst), dst.stride(0), _stream()),
          "sw_scale_cols")
    return dst


def oicr_predict(logits, R, K, refine_k, base_col, round_stride, boxes, reg_weights, scale_clamp, all_scores, all_boxes):
    rw = _floats(reg_weights, 4)
    check(lib.sw_oicr_predict(R, K, refine_k, _p(logits), logits.stride(0), base_col, round_stride, _p(boxes), rw,
                              float(scale_clamp), _p(all_scores), _p(all_boxes), _stream()), "sw_oicr_predict")


def detect_postprocess(all_scores, all_boxes, img_h, img_w, score_thresh, nms_thresh, topk, out=None):
    """-> (count[1] i32, boxes [topk,4], scores [topk], classes [topk] i32, rows [topk] i32) device tensors.  out: optional
    preallocated (count, boxes, scores, classes, rows) — only the first count[0] rows are written (without `out` the rest is zero)"""
    R, K1 = all_scores.shape
    K = K1 - 1
    dev = all_scores.device
    if out is not None:
        cnt, boxes, scores, classes, rows = out
    else:
        cnt = torch.zeros(1, device=dev, dtype=torch.int32)
        boxes = torch.zeros(topk, 4, device=dev); scores = torch.zeros(topk, device=dev)
        classes = torch.zeros(topk, device=dev, dtype=torch.int32); rows = torch.zeros(topk, device=dev, dtype=torch.int32)
    nbytes = int(lib.sw_detect_workspace_bytes(R, K, topk))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    check(lib.sw_detect_postprocess(R, K, _p(all_scores), _p(all_boxes), int(img_h), int(img_w), float(score_thresh),
                                    float(nms_thresh), int(topk), _p(cnt), _p(boxes), _p(scores), _p(classes), _p(rows), _p(ws),
                                    nbytes, _stream()), "sw_detect_postprocess")
    return cnt, boxes, scores, classes, rows


TTA_MERGE_MAX_ROWS, TTA_MERGE_MAX_CLASSES = 2048, 1024


def tta_merge(boxes, scores, classes, counts, view_tab, img_h, img_w, nms_thresh, topk, num_classes, out=None):
    """sw_tta_merge: the views' padded detections boxes (V, T, 4) f32, scores (V, T) f32, classes (V, T) i32, device counts (V,) i32 and
    view_tab (V, 6) f32 = rows of (flip, view width, rx, ry, px, py) -> (count[1] i32, boxes [topk,4], scores [topk], classes [topk] i32,
    src [topk] i32 = union index v * T + slot) device tensors, no host read.  out: optional preallocated (count, boxes, scores, classes,
    src) — only the first count[0] rows are written (without `out` the rest is zero).  count[0] == -1: a count outside [0, T]
    (tta_merge_count raises on it).  V * T > 2048 or num_classes > 1024: ValueError."""
    _need_gpu(boxes, scores, classes, counts, view_tab)
    V, T = scores.shape
    K = int(num_classes)
    if V * T > TTA_MERGE_MAX_ROWS or not 1 <= K <= TTA_MERGE_MAX_CLASSES or topk < 1:
        raise ValueError(f"tta_merge: V * T = {V * T} (limit {TTA_MERGE_MAX_ROWS}), num_classes = {K} (1 .. {TTA_MERGE_MAX_CLASSES}), "
                         f"topk = {topk} (>= 1)")
    if (tuple(boxes.shape) != (V, T, 4) or tuple(classes.shape) != (V, T) or tuple(counts.shape) != (V,) or tuple(view_tab.shape) != (V, 6)
            or boxes.dtype != torch.float32 or scores.dtype != torch.float32 or view_tab.dtype != torch.float32
            or classes.dtype != torch.int32 or counts.dtype != torch.int32
            or not all(t.is_contiguous() for t in (boxes, scores, classes, counts, view_tab)) or boxes.data_ptr() % 16):
        raise ValueError("tta_merge: contiguous boxes (V, T, 4) f32 (16-byte aligned), scores (V, T) f32, classes (V, T) i32, counts (V,) i32, "
                         "view_tab (V, 6) f32 expected")
    dev = scores.device
    if out is not None:
        cnt, dboxes, dscores, dclasses, src = out
        _need_gpu(*out)
    else:
        cnt = torch.zeros(1, device=dev, dtype=torch.int32)
        dboxes = torch.zeros(topk, 4, device=dev); dscores = torch.zeros(topk, device=dev)
        dclasses = torch.zeros(topk, device=dev, dtype=torch.int32); src = torch.zeros(topk, device=dev, dtype=torch.int32)
    rc = lib.sw_tta_merge(V, T, K, _p(boxes), _p(scores), _p(classes), _p(counts), _p(view_tab), int(img_h), int(img_w),
                          float(nms_thresh), int(topk), _p(cnt), _p(dboxes), _p(dscores), _p(dclasses), _p(src), _stream())
    if rc == -6:
        raise ValueError("sw_tta_merge: V * T <= 2048, 1 <= num_classes <= 1024, topk >= 1")
    check(rc, "sw_tta_merge")
    return cnt, dboxes, dscores, dclasses, src


def tta_merge_count(cnt):
    """the one host read of a tta_merge call: its detection count; raises on the poisoned count (-1: a view's count outside [0, T])"""
    n = int(cnt.item())
    if n < 0:
        raise ValueError("tta_merge: a view's detection count lies outside [0, T]")
    return n


# ------------------------------------------------------------------------------------------------ Stage-3 detector (csrc/detector.hip)
def preprocess_pad(img_u8_chw, out_hw4, mean, std):
    """u8 (3, h, w) -> out (H, W, 4) = (img - mean) / std, zero padding (bottom / right) and zero 4th channel"""
    _need_gpu(img_u8_chw, out_hw4)
    h, w = img_u8_chw.shape[1:]
    H, W = out_hw4.shape[:2]
    m, s = _floats(mean, 3), _floats(std, 3)
    check(lib.sw_preprocess_pad(dt(out_hw4), h, w, H, W, _p(img_u8_chw), m, s, _p(out_hw4), _stream()), "sw_preprocess_pad")
    return out_hw4


def stem_conv7x7(x_nhwc4, w_oihw, scale, bias, out):
    n, H, W, _ = x_nhwc4.shape
    check(lib.sw_stem_conv7x7(dt(x_nhwc4), n, H, W, _p(x_nhwc4), _p(w_oihw), _p(scale), _p(bias), _p(out), _stream()), "sw_stem_conv7x7")
    return out


def maxpool3x3s2(x, out):
    n, H, W, C = x.shape
    check(lib.sw_maxpool3x3s2(dt(x), n, H, W, C, _p(x), _p(out), _stream()), "sw_maxpool3x3s2")
    return out


def subsample2x(x, out):
    n, H, W, C = x.shape
    check(lib.sw_subsample2x(dt(x), n, H, W, C, _p(x), _p(out), _stream()), "sw_subsample2x")
    return out


def scatter2x(g, out):
    """out (n, H, W, C) fully written: g (n, ceil(H/2), ceil(W/2), C) at the even pixels, 0 elsewhere"""
    n, H, W, C = out.shape
    check(lib.sw_scatter2x(dt(out), n, H, W, C, _p(g), _p(out), _stream()), "sw_scatter2x")
    return out


def im2col3x3(x, col, stride):
    """x (n, H, W, C) -> col (n * Ho * Wo, >= 9 C) in [tap][c] column order, Ho = (H - 1) // stride + 1 (sw_im2col3x3): with the
    staged [co][tap][ci] weight as B, a 3x3 convolution of stride 1 or 2 is gemm(col, staged.view(cout, 9 C))"""
    _need_gpu(x, col)
    n, H, W, C = x.shape
    assert x.is_contiguous() and col.dim() == 2 and col.stride(1) == 1 and col.dtype == x.dtype
    assert col.shape[0] == n * ((H - 1) // stride + 1) * ((W - 1) // stride + 1) and col.shape[1] >= 9 * C
    check(lib.sw_im2col3x3(dt(x), n, H, W, C, stride, _p(x), _p(col), col.stride(0), _stream()), "sw_im2col3x3")
    return col


def col2im3x3(dcol, dx, stride, relu_ref=None):
    """the adjoint of im2col3x3: dx (n, H, W, C) = the gathered sums of dcol's cells (f32, ascending tap order, rounded once), 0 where
    relu_ref (same shape and dtype as dx) <= 0 (sw_col2im3x3); every element of dx is written"""
    _need_gpu(dcol, dx, relu_ref)
    n, H, W, C = dx.shape
    assert dx.is_contiguous() and dcol.dim() == 2 and dcol.stride(1) == 1 and dcol.dtype == dx.dtype
    assert dcol.shape[0] == n * ((H - 1) // stride + 1) * ((W - 1) // stride + 1) and dcol.shape[1] >= 9 * C
    assert relu_ref is None or (relu_ref.shape == dx.shape and relu_ref.dtype == dx.dtype and relu_ref.is_contiguous())
    check(lib.sw_col2im3x3(dt(dx), n, H, W, C, stride, _p(dcol), dcol.stride(0), _p(relu_ref), _p(dx), _stream()), "sw_col2im3x3")
    return dx


def add_relu(a, b, out, relu=True):
    check(lib.sw_add_relu(dt(a), a.numel(), _p(a), _p(b), _p(out), int(relu), _stream()), "sw_add_relu")
    return out


def upsample2x_add(lateral, top, out):
    n, h, w, C = top.shape
    assert tuple(lateral.shape) == (n, 2 * h, 2 * w, C), (tuple(lateral.shape), tuple(top.shape))
    check(lib.sw_upsample2x_add(dt(top), n, h, w, C, _p(lateral), _p(top), _p(out), _stream()), "sw_upsample2x_add")
    return out


def downsample2x_sum(g, out):
    n, h, w, C = out.shape
    check(lib.sw_downsample2x_sum(dt(g), n, h, w, C, _p(g), _p(out), _stream()), "sw_downsample2x_sum")
    return out


def roi_align_fwd(feat, rois, sel_i32, out, scale, PH=7, PW=7, sampling_ratio=0, n_sel_dev=None):
    """feat (N, H, W, C) of one level; rois (R, 5) f32; sel int32 rows of this level; out (R, C*PH*PW).  n_sel_dev: device int32 [1]
    holding the real length of `sel` (then sel.numel() is only its bound: no host round trip for the level lists)"""
    _need_gpu(feat, rois, sel_i32, out)
    n, H, W, C = feat.shape
    check(lib.sw_roi_align_fwd(dt(feat), H, W, C, PH, PW, float(scale), sampling_ratio, _p(feat), _p(rois), _p(sel_i32),
                               sel_i32.numel(), _p(n_sel_dev), _p(out), out.stride(0), _stream()), "sw_roi_align_fwd")
    return out


def roi_align_bwd(gout, rois, sel_i32, dfeat_f32, scale, PH=7, PW=7, sampling_ratio=0, n_sel_dev=None):
    _need_gpu(gout, rois, sel_i32, dfeat_f32)
    n, H, W, C = dfeat_f32.shape
    check(lib.sw_roi_align_bwd(dt(gout), H, W, C, PH, PW, float(scale), sampling_ratio, _p(gout), gout.stride(0), _p(rois),
                               _p(sel_i32), sel_i32.numel(), _p(n_sel_dev), _p(dfeat_f32), _stream()), "sw_roi_align_bwd")
    return dfeat_f32


def roi_align_bwd_fx(gout, rois, sel_i32, acc_i64, scale, gout_absmax, PH=7, PW=7, sampling_ratio=0, n_sel_dev=None):
    """the deterministic ROIAlign backward (sw_roi_align_bwd_fx): acc_i64 (N, H, W, C) int64, zero-filled, collects the level's
    contributions as 64-bit fixed-point integers scaled by 2^(40 - e), where gout_absmax = f * 2^e with
    f in [0.5, 1) (device scalar from ops.absmax(gout)); fx_to_float turns it into the gradient map"""
    _need_gpu(gout, rois, sel_i32, acc_i64, gout_absmax)
    assert acc_i64.dtype == torch.int64 and acc_i64.is_contiguous()
    n, H, W, C = acc_i64.shape
    check(lib.sw_roi_align_bwd_fx(dt(gout), H, W, C, PH, PW, float(scale), sampling_ratio, _p(gout), gout.stride(0), _p(rois),
                                  _p(sel_i32), sel_i32.numel(), _p(n_sel_dev), _p(gout_absmax), _p(acc_i64), _stream()), "sw_roi_align_bwd_fx")


def fx_to_float(acc_i64, absmax, out):
    """out[i] = acc_i64[i] * 2^(e - 40), absmax = f * 2^e with f in [0.5, 1) (sw_fx_to_float); out f32 or bf16, same element count"""
    _need_gpu(acc_i64, absmax, out)
    assert acc_i64.dtype == torch.int64 and out.numel() == acc_i64.numel() and out.is_contiguous()
    check(lib.sw_fx_to_float(dt(out), acc_i64.numel(), _p(acc_i64), _p(absmax), _p(out), _stream()), "sw_fx_to_float")
    return out


def wsddn_scores_bwd(logits, K, g_scores, dlogits):
    """analytic backward of scores = softmax(C, 1) * softmax(D, 0) for ONE image's rows (sw_wsddn_scores_bwd): logits (R, >= 2K) f32,
    g_scores (R, K) f32 -> dlogits[:, :2K]"""
    _need_gpu(logits, g_scores, dlogits)
    R = logits.shape[0]
    ws = torch.empty(int(lib.sw_wsddn_scores_bwd_workspace_floats(R, K)), device=logits.device, dtype=torch.float32)
    check(lib.sw_wsddn_scores_bwd(R, K, _p(logits), logits.stride(0), _p(g_scores), g_scores.stride(0), _p(dlogits), dlogits.stride(0),
                                  _p(ws), _stream()), "sw_wsddn_scores_bwd")
    return dlogits


def scale_col_blocks(src, dst, split, g0, g1):
    """dst[:, :split] = src[:, :split] * g0, dst[:, split:] = src[:, split:] * g1 (device scalars); src / dst (M, N) f32 views of
    buffers with one row pitch, padding columns of dst zeroed"""
    _need_gpu(src, dst, g0, g1)
    M, N = src.shape
    assert src.stride(0) == dst.stride(0) and src.dtype == dst.dtype == torch.float32
    check(lib.sw_scale_col_blocks(M, N, int(split), _p(src), src.stride(0), _p(g0), _p(g1), _p(dst), _stream()), "sw_scale_col_blocks")
    return dst


def convert_flat(src_f32, dtype):
    """a float32 tensor in another compute dtype (same shape), through sw_convert_2d"""
    _need_gpu(src_f32)
    out = torch.empty(src_f32.shape, device=src_f32.device, dtype=dtype)
    c = src_f32.shape[-1]
    r = src_f32.numel() // c
    check(lib.sw_convert_2d(dt(out), r, c, _p(src_f32), c, _p(out), c, _stream()), "sw_convert_2d")
    return out


def rpn_unpack(y, N, A, hw_per_level):
    """y (rows, ld) f32, the RPN head's packed GEMM output -> logits (N, At), deltas (N, At, 4) in anchor order (sw_rpn_unpack)"""
    _need_gpu(y)
    L = len(hw_per_level)
    At = A * int(sum(hw_per_level))
    hw = (ctypes.c_int * L)(*[int(v) for v in hw_per_level])
    logits = torch.empty(N, At, device=y.device); deltas = torch.empty(N, At, 4, device=y.device)
    check(lib.sw_rpn_unpack(N, L, A, hw, _p(y), y.stride(0), _p(logits), _p(deltas), _stream()), "sw_rpn_unpack")
    return logits, deltas


def rpn_unpack_bwd(dlogits, ddeltas, N, A, hw_per_level, rows, ld, device, g_logits=None, g_deltas=None):
    """gradient of rpn_unpack's input: dy (rows, ld) f32 from dlogits (N, At) / ddeltas (N, At, 4), each times a device scalar"""
    L = len(hw_per_level)
    hw = (ctypes.c_int * L)(*[int(v) for v in hw_per_level])
    dy = torch.empty(rows, ld, device=device)
    check(lib.sw_rpn_unpack_bwd(N, L, A, hw, _p(dlogits), _p(ddeltas), _p(g_logits), _p(g_deltas), _p(dy), ld, _stream()),
          "sw_rpn_unpack_bwd")
    return dy


def roi_assign_levels(boxes_base, row_cnt, box_off_floats):
    """dense ROI rows + FPN levels (sw_roi_assign_levels).  boxes_base: a f32 tensor the images' box blocks live in; image i contributes
    row_cnt[i] boxes starting box_off_floats[i] floats into it.  -> rois (R, 5), level_of (R,), sel (4, R) int32, sel_cnt (4,) int32"""
    _need_gpu(boxes_base)
    n = len(row_cnt)
    R = int(sum(row_cnt))
    if n > 64 or R > (1 << 20):
        raise ValueError(f"sw_roi_assign_levels takes at most 64 images and 2^20 boxes per call (got {n} images, {R} boxes): its per-level "
                         "row lists run over all images of the call; pool larger batches in several calls")
    dev = boxes_base.device
    rois = torch.empty(R, 5, device=dev); lv = torch.empty(R, device=dev, dtype=torch.int32)
    sel = torch.empty(4, max(R, 1), device=dev, dtype=torch.int32); cnt = torch.empty(4, device=dev, dtype=torch.int32)
    rc = (ctypes.c_int * n)(*[int(v) for v in row_cnt]); bo = (ctypes.c_long * n)(*[int(v) for v in box_off_floats])
    check(lib.sw_roi_assign_levels(n, rc, bo, _p(boxes_base), _p(rois), _p(lv), _p(sel), _p(cnt), _stream()), "sw_roi_assign_levels")
    return rois, lv, sel, cnt


def rpn_select_pack(logits, deltas, anchors, pre_topk, weights, scale_clamp, img_hw_dev, ints_out=None):
    """RPN proposal selection up to the NMS (sw_rpn_select_pack).  anchors: per level (n_l, 4); img_hw_dev (N, 2) int32 device;
    logits / deltas: either per-level lists ((N, n_l) / (N, n_l, 4) f32, each dense) or ONE pair (N, At) / (N, At, 4) in anchor order
    (ops.rpn_unpack) whose column ranges are the levels.  -> cand_scores (N, L * pre_topk, L + 1), cand_boxes (N, L * pre_topk, 4 L) in
    sw_detect_postprocess's form (class = level), finite (N,) int32 (a slice of ints_out when given)"""
    L = len(anchors)
    dev = anchors[0].device
    n_list = [int(a.shape[0]) for a in anchors]
    if isinstance(logits, torch.Tensor):
        N, At = logits.shape
        assert At == sum(n_list) and logits.is_contiguous() and deltas.is_contiguous() and logits.dtype == deltas.dtype == torch.float32
        _need_gpu(logits, deltas)
        off, lp, dp = 0, [], []
        for n in n_list:
            lp.append(logits.data_ptr() + 4 * off); dp.append(deltas.data_ptr() + 16 * off); off += n
        stride = At
    else:
        N = logits[0].shape[0]
        for t in list(logits) + list(deltas):
            _need_gpu(t)
            assert t.dtype == torch.float32 and t.is_contiguous()
        lp, dp, stride = [t.data_ptr() for t in logits], [t.data_ptr() for t in deltas], 0
    for a in anchors:
        assert a.dtype == torch.float32 and a.is_contiguous()
    n_l = (ctypes.c_int * L)(*n_list)
    arr = lambda ps: (ctypes.c_void_p * L)(*ps)
    nbytes = int(lib.sw_rpn_select_workspace_bytes(N, L, n_l))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    rows = L * pre_topk
    sc = torch.empty(N, rows, L + 1, device=dev); bx = torch.empty(N, rows, 4 * L, device=dev)
    fin = ints_out if ints_out is not None else torch.empty(N, device=dev, dtype=torch.int32)
    sel = torch.empty(N * L, pre_topk, device=dev, dtype=torch.int32)
    rw = _floats(weights, 4)
    check(lib.sw_rpn_select_pack(N, L, arr(lp), arr(dp), arr([a.data_ptr() for a in anchors]), n_l, stride, int(pre_topk), rw,
                                 float(scale_clamp), _p(img_hw_dev), _p(sc), _p(bx), _p(fin), _p(sel), _p(ws), nbytes, _stream()),
          "sw_rpn_select_pack")
    return sc, bx, fin


def rpn_label_anchors(anchors, gt_boxes, gt_counts, seeds, batch_size, max_pos, thr_lo=0.3, thr_hi=0.7):
    """RPN anchor labels + matched boxes (sw_rpn_label_anchors).  anchors (A, 4); gt_boxes (sum G_i, 4) the images' boxes back to back;
    gt_counts: host ints per image; seeds: host ints, (positives, negatives) per image.  -> labels int8 (N, A), matched (N, A, 4)"""
    _need_gpu(anchors)
    N, A = len(gt_counts), anchors.shape[0]
    dev = anchors.device
    tot = int(sum(gt_counts))
    assert anchors.dtype == torch.float32 and anchors.is_contiguous() and len(seeds) == 2 * N
    assert tot == 0 or (gt_boxes.is_cuda and gt_boxes.dtype == torch.float32 and gt_boxes.is_contiguous() and gt_boxes.shape[0] == tot)
    nbytes = int(lib.sw_rpn_label_workspace_bytes(N, A, tot))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    labels = torch.empty(N, A, device=dev, dtype=torch.int8); matched = torch.empty(N, A, 4, device=dev)
    cnt = (ctypes.c_int * N)(*[int(c) for c in gt_counts])
    sd = (ctypes.c_uint64 * (2 * N))(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in seeds])
    check(lib.sw_rpn_label_anchors(N, A, _p(anchors), _p(gt_boxes) if tot else None, cnt, float(thr_lo), float(thr_hi), int(batch_size),
                                   int(max_pos), sd, _p(labels), _p(matched), _p(ws), nbytes, _stream()), "sw_rpn_label_anchors")
    return labels, matched


def roi_label_sample(p_cnt_dev, proposals, gt_boxes, gt_classes_i32, gt_counts, seeds, append_gt, iou_thresh, num_classes, batch_size, max_pos):
    """ROI-head matching + sampling (sw_roi_label_sample).  proposals (N, p_stride, 4) with device counts p_cnt_dev (N,) int32; gt_boxes
    (sum G_i, 4) / gt_classes_i32 back to back, gt_counts host ints.  -> count (N,) i32, index / classes (N, batch) i32, both (2, N, batch, 4)
    = (sampled boxes, their matched gt boxes): image i's sampled rows are the first count[i] (foreground list, then background, each in
    random-key order)"""
    _need_gpu(p_cnt_dev, proposals)
    N, ps = proposals.shape[0], proposals.shape[1]
    dev = proposals.device
    tot = int(sum(gt_counts))
    assert proposals.dtype == torch.float32 and proposals.is_contiguous() and p_cnt_dev.dtype == torch.int32 and len(seeds) == 2 * N
    offs, r = [], 0
    for c in gt_counts:
        offs.append(r); r += int(c)
    g_off = (ctypes.c_int * N)(*offs); g_cnt = (ctypes.c_int * N)(*[int(c) for c in gt_counts])
    sd = (ctypes.c_uint64 * (2 * N))(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in seeds])
    cnt = torch.empty(N, device=dev, dtype=torch.int32)
    idx = torch.empty(N, batch_size, device=dev, dtype=torch.int32); cls = torch.empty(N, batch_size, device=dev, dtype=torch.int32)
    both = torch.empty(2, N, batch_size, 4, device=dev)                 # [0] the sampled boxes, [1] their matched gt boxes
    check(lib.sw_roi_label_sample(N, _p(p_cnt_dev), ps, _p(proposals), g_off, g_cnt, _p(gt_boxes) if tot else None,
                                  _p(gt_classes_i32) if tot else None, int(bool(append_gt)), float(iou_thresh), int(num_classes),
                                  int(batch_size), int(max_pos), sd, batch_size, _p(cnt), _p(idx), _p(cls), _p(both[0]), _p(both[1]),
                                  _stream()), "sw_roi_label_sample")
    return cnt, idx, cls, both


def rpn_loss(logits, deltas, labels_i8, anchors, matched_gt, weights, inv_norm, losses2, dlogits=None, ddeltas=None):
    """logits (n,), deltas (n, 4), labels int8 (n,), anchors (A, 4) repeating over the images, matched_gt (n, 4) -> losses2 (2,)"""
    _need_gpu(logits, deltas, labels_i8, anchors, matched_gt, losses2)
    rw = _floats(weights, 4)
    ws = torch.empty(int(lib.sw_rpn_loss_workspace_floats()), device=logits.device, dtype=torch.float32)
    check(lib.sw_rpn_loss(logits.numel(), anchors.shape[0], _p(logits), _p(deltas), _p(labels_i8), _p(anchors), _p(matched_gt), rw,
                          float(inv_norm), _p(losses2), _p(dlogits), _p(ddeltas), _p(ws), _stream()), "sw_rpn_loss")
    return losses2


DET_LOSS_TYPES = {"smooth_l1": 0, "smooth_l1_mean": 1}


def det_loss_per_image(rpn_logits, rpn_deltas, rpn_labels_i8, anchors, rpn_matched, rpn_weights, rpn_batch_size, rpn_loss_type,
                       roi_logits, K, roi_classes_i32, roi_boxes, roi_gt_boxes, roi_counts_i32, roi_batch_size, roi_weights, gamma,
                       roi_loss_type):
    """Each image's four detector losses as if it were alone in its batch (sw_det_loss_per_image): rpn_logits (N, A), rpn_deltas /
    rpn_matched (N, A, 4), rpn_labels int8 (N, A), anchors (A, 4); roi_logits (R, >= 5K+1) packed [cls | box], roi_classes (R,),
    roi_boxes / roi_gt_boxes (R, 4), image i's rows after those of images < i, roi_counts (N,) int32 on the device (no host read),
    each <= roi_batch_size (the ROI sampler's batch_size_per_image; a larger count gives NaN).
    Loss types: "smooth_l1" / "smooth_l1_mean"; gamma 0 = cross-entropy.  -> (N, 5) f32: loss_cls, loss_box_reg, loss_rpn_cls,
    loss_rpn_loc, their sum."""
    _need_gpu(rpn_logits, rpn_deltas, rpn_labels_i8, anchors, rpn_matched, roi_logits, roi_classes_i32, roi_boxes, roi_gt_boxes,
              roi_counts_i32)
    N, A = rpn_logits.shape
    R = roi_logits.shape[0]
    assert rpn_logits.dtype == torch.float32 and rpn_deltas.dtype == torch.float32 and rpn_matched.dtype == torch.float32
    assert rpn_labels_i8.dtype == torch.int8 and anchors.dtype == torch.float32 and roi_logits.dtype == torch.float32
    assert roi_classes_i32.dtype == torch.int32 and roi_counts_i32.dtype == torch.int32
    assert rpn_deltas.shape == (N, A, 4) and rpn_matched.shape == (N, A, 4) and rpn_labels_i8.shape == (N, A) and anchors.shape == (A, 4)
    assert roi_logits.dim() == 2 and roi_logits.shape[1] >= 5 * K + 1 and roi_logits.stride(1) == 1
    assert roi_classes_i32.shape == (R,) and roi_boxes.shape == (R, 4) and roi_gt_boxes.shape == (R, 4) and roi_counts_i32.shape == (N,)
    for t in (rpn_logits, rpn_deltas, rpn_labels_i8, anchors, rpn_matched, roi_classes_i32, roi_boxes, roi_gt_boxes, roi_counts_i32):
        assert t.is_contiguous()
    out = torch.empty(N, 5, device=rpn_logits.device, dtype=torch.float32)
    ws = torch.empty(max(int(lib.sw_det_loss_workspace_floats(N, A, int(roi_batch_size))), 1), device=rpn_logits.device,
                     dtype=torch.float32)
    rw = _floats(rpn_weights, 4); bw = _floats(roi_weights, 4)
    check(lib.sw_det_loss_per_image(N, A, _p(rpn_logits), _p(rpn_deltas), _p(rpn_labels_i8), _p(anchors), _p(rpn_matched), rw,
                                    int(rpn_batch_size), DET_LOSS_TYPES[rpn_loss_type], _p(roi_logits), roi_logits.stride(0), int(K),
                                    _p(roi_classes_i32), _p(roi_boxes), _p(roi_gt_boxes), _p(roi_counts_i32), R, int(roi_batch_size), bw, float(gamma),
                                    DET_LOSS_TYPES[roi_loss_type], _p(out), _p(ws), _stream()), "sw_det_loss_per_image")
    return out


def pgf_keep(det_off, boxes, scores, classes, K, gt_mask, diff_mask, t_keep, t_con, use_diff):
    """Stage-2 pseudo-ground-truth filtering of one split (sw_pgf_keep): det_off [n_img + 1] i64, boxes [N, 4] f64, scores [N] f64,
    classes [N] i32 in [0, K), gt_mask [n_img, (K + 31) // 32] and diff_mask [(K + 31) // 32] i32 class bitmasks, all on the GPU.
    -> packed u8 [32 + N]: bytes [0, 32) the four int64 counts (before the class filter, after it, after the keep stage, after the
    containment stage), bytes [32, 32 + N) the keep flags — one tensor, so the host reads everything with one copy."""
    _need_gpu(det_off, boxes, scores, classes, gt_mask, diff_mask)
    n_img, n = det_off.numel() - 1, boxes.shape[0]
    words = (K + 31) // 32
    assert det_off.dtype == torch.int64 and boxes.dtype == torch.float64 and scores.dtype == torch.float64
    assert classes.dtype == torch.int32 and gt_mask.dtype == torch.int32 and diff_mask.dtype == torch.int32
    assert boxes.shape == (n, 4) and scores.shape == (n,) and classes.shape == (n,) and n_img >= 0
    assert gt_mask.shape == (n_img, words) and diff_mask.shape == (words,)
    for t in (det_off, boxes, scores, classes, gt_mask, diff_mask):
        assert t.is_contiguous()
    packed = torch.empty(32 + n, device=boxes.device, dtype=torch.uint8)
    workspace = torch.empty(max(n, 1), device=boxes.device, dtype=torch.uint8)
    check(lib.sw_pgf_keep(n_img, _p(det_off), _p(boxes), _p(scores), _p(classes), int(K), _p(gt_mask), _p(diff_mask),
                          float(t_keep), float(t_con), int(bool(use_diff)), ctypes.c_void_p(packed.data_ptr() + 32), _p(workspace),
                          _p(packed), _stream()), "sw_pgf_keep")
    return packed


PGF_LDS_CAP, PGF_MAX_CLASSES = 256, 256                                 # SW_PGF_LDS_CAP / SW_PGF_MAX_CLASSES
PGF_SWEEP_MAX_KEEP, PGF_SWEEP_MAX_CON, PGF_SWEEP_MAX_IOU = 32, 32, 10   # SW_PGF_SWEEP_MAX_*
PGF_SWEEP_WS_WORDS = 12                                                 # SW_PGF_SWEEP_WS_WORDS


def pgf_sweep_layout(nk, nc, nt, K, guard=0):
    """Where the four tables of sw_pgf_sweep lie in the packed int64 tensor, `guard` untouched words before, between and after
    them.  -> ({"kept": (offset, shape), "tp": ..., "ign": ..., "npos": ...}, total words)"""
    shapes = (("kept", (nk, nc, K)), ("tp", (nt, nk, nc, K)), ("ign", (nt, nk, nc, K)), ("npos", (K,)))
    at, out = guard, {}
    for name, shape in shapes:
        size = 1
        for s in shape:
            size *= s
        out[name] = (at, shape)
        at += size + guard
    return out, at


def pgf_sweep_unpack(host, nk, nc, nt, K, guard=0):
    """the four tables as views of the packed tensor's host copy (a numpy int64 array)"""
    layout, total = pgf_sweep_layout(nk, nc, nt, K, guard)
    assert host.shape == (total,)
    out = {}
    for name, (at, shape) in layout.items():
        size = 1
        for s in shape:
            size *= s
        out[name] = host[at:at + size].reshape(shape)
    return out


def pgf_sweep(det_off, boxes, scores, classes, K, gt_mask, diff_mask, use_diff, t_keep, t_con, iou, gt_off, gt_box, gt_cls, gt_ign,
              xywh, plus_one, guard=0, out=None):
    """The Stage-2 filter at every cell of t_keep x t_con with voc_eval's matching at every iou, counted per cell and class
    (sw_pgf_sweep).  Detections and masks as for pgf_keep; t_keep (<= 32), t_con (<= 32), iou (<= 10): sequences of finite floats;
    gt_off [n_img + 1] i64, gt_box [G, 4] f64 corners, gt_cls [G] i32, gt_ign [G] u8 on the GPU.  `out` (int64, pgf_sweep_layout's
    total words) may be passed in: tests fill it with sentinels around the tables.
    -> packed int64 tensor on the GPU holding kept [nk, nc, K], tp [nt, nk, nc, K], ign [nt, nk, nc, K] and npos [K] — one tensor,
    so the host reads everything with one copy; pgf_sweep_unpack splits its host copy."""
    _need_gpu(det_off, boxes, scores, classes, gt_mask, diff_mask, gt_off, gt_box, gt_cls, gt_ign, out)
    n_img, n, G = det_off.numel() - 1, boxes.shape[0], gt_box.shape[0]
    words = (K + 31) // 32
    assert det_off.dtype == torch.int64 and boxes.dtype == torch.float64 and scores.dtype == torch.float64
    assert classes.dtype == torch.int32 and gt_mask.dtype == torch.int32 and diff_mask.dtype == torch.int32
    assert gt_off.dtype == torch.int64 and gt_box.dtype == torch.float64 and gt_cls.dtype == torch.int32
    assert gt_ign.dtype == torch.uint8
    assert boxes.shape == (n, 4) and scores.shape == (n,) and classes.shape == (n,) and n_img >= 0
    assert gt_mask.shape == (n_img, words) and diff_mask.shape == (words,)
    assert gt_off.shape == (n_img + 1,) and gt_box.shape == (G, 4) and gt_cls.shape == (G,) and gt_ign.shape == (G,)
    for t in (det_off, boxes, scores, classes, gt_mask, diff_mask, gt_off, gt_box, gt_cls, gt_ign):
        assert t.is_contiguous()
    nk, nc, nt = len(t_keep), len(t_con), len(iou)
    # sizes the entry point refuses still need a tensor to pass: lay it out as if they were 1
    layout, total = pgf_sweep_layout(max(nk, 1), max(nc, 1), max(nt, 1), max(int(K), 1), guard)
    if out is None:
        out = torch.empty(total, device=boxes.device, dtype=torch.int64)
    assert out.dtype == torch.int64 and out.shape == (total,) and out.is_contiguous()
    workspace = torch.empty(max(n, 1) * PGF_SWEEP_WS_WORDS, device=boxes.device, dtype=torch.int32)

    def host(values):
        return (ctypes.c_double * max(len(values), 1))(*[float(v) for v in values])

    def table(name):
        return ctypes.c_void_p(out.data_ptr() + 8 * layout[name][0])

    check(lib.sw_pgf_sweep(n_img, n, _p(det_off), _p(boxes), _p(scores), _p(classes), int(K), _p(gt_mask), _p(diff_mask),
                           int(bool(use_diff)), nk, host(t_keep), nc, host(t_con), nt, host(iou), _p(gt_off), _p(gt_box),
                           _p(gt_cls), _p(gt_ign), int(bool(xywh)), int(bool(plus_one)), _p(workspace), table("kept"), table("tp"),
                           table("ign"), table("npos"), _stream()), "sw_pgf_sweep")
    return out


VOC_THRESHOLDS = 10


def voc_eval(det_off, det_img, det_box, gt_off, gt_box, gt_diff, npos, npos_im, thr, t11):
    """VOC AP and CorLoc of one split at every IoU threshold (sw_voc_eval), all inputs on the GPU: det_off [K + 1] i64 (detections
    grouped by class in rank order), det_img [N] i32, det_box [N, 4] f64, gt_off [n_img * K + 1] i64 (ground truth per (image,
    class)), gt_box [G, 4] f64, gt_diff [G] u8, npos [K] / npos_im [K] i64, thr [10] f64 IoU thresholds, t11 [11] f64 recall levels.
    -> f64 [3, K, 10] on the GPU: area AP, 11-point AP, CorLoc (the caller copies it back once)."""
    _need_gpu(det_off, det_img, det_box, gt_off, gt_box, gt_diff, npos, npos_im, thr, t11)
    K, N, G = det_off.numel() - 1, det_img.numel(), gt_diff.numel()
    n_img = (gt_off.numel() - 1) // K
    assert det_off.dtype == torch.int64 and det_img.dtype == torch.int32 and det_box.dtype == torch.float64
    assert gt_off.dtype == torch.int64 and gt_box.dtype == torch.float64 and gt_diff.dtype == torch.uint8
    assert npos.dtype == torch.int64 and npos_im.dtype == torch.int64 and thr.dtype == torch.float64 and t11.dtype == torch.float64
    assert det_box.shape == (N, 4) and gt_box.shape == (G, 4) and gt_off.numel() == n_img * K + 1
    assert npos.shape == (K,) and npos_im.shape == (K,) and thr.shape == (VOC_THRESHOLDS,) and t11.shape == (11,)
    for t in (det_off, det_img, det_box, gt_off, gt_box, gt_diff, npos, npos_im, thr, t11):
        assert t.is_contiguous()
    nbytes = lib.sw_voc_eval_workspace_bytes(K, n_img, N, G)
    assert nbytes > 0, "sw_voc_eval_workspace_bytes"
    ws, ws_p = _workspace256(nbytes, det_box.device)
    out = torch.empty(3, K, VOC_THRESHOLDS, device=det_box.device, dtype=torch.float64)
    check(lib.sw_voc_eval(K, n_img, N, G, _p(det_off), _p(det_img), _p(det_box), _p(gt_off), _p(gt_box), _p(gt_diff), _p(npos),
                          _p(npos_im), _p(thr), _p(t11), _p(out), ws_p, _stream()), "sw_voc_eval")
    return out


COCO_THRESHOLDS, COCO_RECALLS, COCO_AREAS, COCO_MAXDETS = 10, 101, 4, 3
COCO_LDS_DOUBLES = 1600                           # SW_COCO_LDS_DOUBLES
COCO_MAX_CLASSES = 4096                           # SW_COCO_MAX_CLASSES
COCO_WS_HEADER = 256                              # SW_COCO_WS_HEADER


def coco_eval(pair_off, pair_gt, pair_ws, ws_words, det_box, gt_off, gt_box, gt_area, gt_flags, area_rng, iou_thr, rec_thr, max_dets,
              cat_off, order, det_rank, det_score, npig, lds_doubles=COCO_LDS_DOUBLES, match=None, out=None):
    """COCO bbox matching and accumulation of one split (sw_coco_eval; the layouts are in include/soswsod_hip.h), all inputs on the
    GPU: pair_off [P + 1] / pair_gt [P] / pair_ws [P] i64, det_box [N, 4] f64 XYWH, gt_off i64, gt_box [G, 4] f64, gt_area [G] f64,
    gt_flags [G] u8, area_rng [4, 2] / iou_thr [10] / rec_thr [101] f64, max_dets [3] i32, cat_off [K + 1] i64, order [N] i32,
    det_rank [N] u8, det_score [N] f64, npig [K, 4] i64.  ws_words: the 8-byte words the pairs outside the LDS path need in all
    (pair_ws holds each one's offset in words).  match [N, 2] u64-as-i64 and out f64 [2 * 10 * 101 * K * 12 + 10 * K * 12] may be
    passed in (tests fill them with sentinels).
    -> (out, match) on the GPU: out is precision [10, 101, K, 4, 3], scores [10, 101, K, 4, 3], recall [10, K, 4, 3] flattened one
    after the other (the caller copies it back once)."""
    ts = (pair_off, pair_gt, pair_ws, det_box, gt_off, gt_box, gt_area, gt_flags, area_rng, iou_thr, rec_thr, max_dets, cat_off,
          order, det_rank, det_score, npig)
    _need_gpu(*ts)
    K, N, P, G = cat_off.numel() - 1, det_score.numel(), pair_gt.numel(), gt_flags.numel()
    for t in (pair_off, pair_gt, pair_ws, gt_off, cat_off, npig):
        assert t.dtype == torch.int64
    for t in (det_box, gt_box, gt_area, area_rng, iou_thr, rec_thr, det_score):
        assert t.dtype == torch.float64
    assert gt_flags.dtype == torch.uint8 and det_rank.dtype == torch.uint8 and max_dets.dtype == torch.int32
    assert order.dtype == torch.int32
    assert pair_off.shape == (P + 1,) and pair_ws.shape == (P,) and det_box.shape == (N, 4) and gt_box.shape == (G, 4)
    assert gt_area.shape == (G,) and order.shape == (N,) and det_rank.shape == (N,) and npig.shape == (K, COCO_AREAS)
    assert area_rng.shape == (COCO_AREAS, 2) and iou_thr.shape == (COCO_THRESHOLDS,) and rec_thr.shape == (COCO_RECALLS,)
    assert max_dets.shape == (COCO_MAXDETS,) and K >= 1 and ws_words >= 0
    for t in ts:
        assert t.is_contiguous()
    n_cell = COCO_THRESHOLDS * K * COCO_AREAS * COCO_MAXDETS
    n_out = 2 * COCO_RECALLS * n_cell + n_cell
    dev = det_box.device
    if out is None:
        out = torch.empty(n_out, device=dev, dtype=torch.float64)
    if match is None:
        match = torch.empty(N, 2, device=dev, dtype=torch.int64)
    assert out.is_cuda and match.is_cuda and out.dtype == torch.float64 and match.dtype == torch.int64
    assert out.shape == (n_out,) and match.shape == (N, 2) and out.is_contiguous() and match.is_contiguous()
    ws_bytes = COCO_WS_HEADER + 8 * int(ws_words)
    ws, ws_p = _workspace256(ws_bytes, dev)
    check(lib.sw_coco_eval(K, N, P, _p(pair_off), _p(pair_gt), _p(pair_ws), ws_bytes, int(lds_doubles), _p(det_box), _p(gt_off),
                           _p(gt_box), _p(gt_area), _p(gt_flags), _p(area_rng), _p(iou_thr), _p(rec_thr), _p(max_dets), _p(cat_off),
                           _p(order), _p(det_rank), _p(det_score), _p(npig), _p(match), _p(out), ws_p, _stream()), "sw_coco_eval")
    return out, match


PROPOSAL_RECALL_MAX_CUTS, PROPOSAL_RECALL_MAX_THRESHOLDS = 16, 16      # SW_PROPOSAL_RECALL_MAX_CUTS / _MAX_THRESHOLDS
PROPOSAL_RECALL_LDS_BOXES = 1024                                        # SW_PROPOSAL_RECALL_LDS_BOXES


def proposal_recall(prop_off, prop_box, gt_off, gt_box, cuts, thr, ovmax=None, jmax=None):
    """Best overlap of every ground-truth box with the first cuts[c] ranked proposals of its image, for every cut at once, and the
    boxes recalled at every threshold (sw_proposal_recall), all inputs on the GPU: prop_off / gt_off [n_img + 1] i64 (CSR over
    images), prop_box [P, 4] / gt_box [G, 4] f64 xyxy, cuts [n_cut <= 16] i32 strictly ascending and >= 1, thr [n_thr <= 16] f64.
    ovmax [>= G, n_cut] f64 and jmax [>= G, n_cut] i32 may be passed in (tests fill them with sentinels; only the first G rows of
    images that have ground truth are written).
    -> (ovmax, jmax, cnt_yes [n_cut, n_thr] i64) on the GPU."""
    _need_gpu(prop_off, prop_box, gt_off, gt_box, cuts, thr, ovmax, jmax)
    n_img, P, G, n_cut, n_thr = prop_off.numel() - 1, prop_box.shape[0], gt_box.shape[0], cuts.numel(), thr.numel()
    assert prop_off.dtype == torch.int64 and gt_off.dtype == torch.int64 and cuts.dtype == torch.int32
    assert prop_box.dtype == torch.float64 and gt_box.dtype == torch.float64 and thr.dtype == torch.float64
    assert n_img >= 0 and gt_off.shape == (n_img + 1,) and prop_off.shape == (n_img + 1,)
    assert prop_box.shape == (P, 4) and gt_box.shape == (G, 4) and cuts.shape == (n_cut,) and thr.shape == (n_thr,)
    assert 1 <= n_cut <= PROPOSAL_RECALL_MAX_CUTS and 1 <= n_thr <= PROPOSAL_RECALL_MAX_THRESHOLDS
    c = cuts.tolist()          # a copy to the host: cuts out of order would give wrong rows, not an error
    assert c[0] >= 1 and all(a < b for a, b in zip(c, c[1:])), f"cuts {c} must be >= 1 and strictly ascending"
    dev = prop_box.device
    if ovmax is None:
        ovmax = torch.empty(G, n_cut, device=dev, dtype=torch.float64)
    if jmax is None:
        jmax = torch.empty(G, n_cut, device=dev, dtype=torch.int32)
    assert ovmax.dtype == torch.float64 and jmax.dtype == torch.int32
    assert ovmax.dim() == 2 and ovmax.shape[0] >= G and ovmax.shape[1] == n_cut and jmax.shape == ovmax.shape
    for t in (prop_off, prop_box, gt_off, gt_box, cuts, thr, ovmax, jmax):
        assert t.is_contiguous()
    cnt_yes = torch.empty(n_cut, n_thr, device=dev, dtype=torch.int64)
    check(lib.sw_proposal_recall(n_img, _p(prop_off), _p(prop_box), _p(gt_off), _p(gt_box), n_cut, _p(cuts), n_thr, _p(thr),
                                 _p(ovmax), _p(jmax), _p(cnt_yes), _stream()), "sw_proposal_recall")
    return ovmax, jmax, cnt_yes


BOXAR_MAX_AREAS, BOXAR_MAX_LIMITS, BOXAR_MAX_THRESHOLDS = 8, 8, 16      # SW_BOXAR_MAX_AREAS / _MAX_LIMITS / _MAX_THRESHOLDS
BOXAR_LDS_BOXES, BOXAR_LDS_GT = 1024, 128                               # SW_BOXAR_LDS_BOXES / SW_BOXAR_LDS_GT
BOXAR_STATUS = {1: "the image offsets decrease or leave their arrays", 2: "item_off is not the layout of this split",
                3: "an item needs more workspace than was given"}       # SW_BOXAR_BAD_OFFSETS / _BAD_LAYOUT / _WORKSPACE


def box_proposal_ar(prop_off, prop_box, gt_off, gt_box, gt_area, area_rng, limits, thr, item_off, overlap=None, match_gt=None,
                    match_box=None, max_boxes=None, max_props=None, check_offsets=True):
    """One-to-one greedy coverage of every image's ground truth by its ranked proposals, for every (limit, area range) at once, and
    the boxes covered at every threshold (sw_box_proposal_ar; the layout is in include/soswsod_hip.h).  On the GPU: prop_off /
    gt_off [n_img + 1] i64 (CSR over images), prop_box [P, 4] f32 xyxy in rank order, gt_box [G, 4] f32, gt_area [G] f32,
    item_off [L * A * n_img + 1] i64.  On the host (sequences): area_rng [A <= 8][2], limits [L <= 8] (0: no limit), thr [T <= 16].
    overlap f32 / match_gt i32 / match_box i32 [>= item_off[-1]] may be passed in (tests fill them with sentinels; only the
    elements of items are written).  max_boxes / max_props: the largest ground-truth count of an image and the largest number of
    proposals an item reads, which size the workspace; read from the offsets when not given.  check_offsets: refuse offsets that
    decrease or leave their arrays with ValueError before the launch (one device-to-host copy; the kernel skips such an image and
    reports it in status either way).
    -> (overlap, match_gt, match_box, cnt_yes [L, A, T] i64, status [1] i32) on the GPU; status is 0 after a clean launch, else a
    key of BOXAR_STATUS."""
    _need_gpu(prop_off, prop_box, gt_off, gt_box, gt_area, item_off, overlap, match_gt, match_box)
    n_img, P, G = prop_off.numel() - 1, prop_box.shape[0], gt_box.shape[0]
    area_rng = [[float(lo), float(hi)] for lo, hi in area_rng]
    limits = [int(v) for v in limits]
    thr = [float(t) for t in thr]
    A, L, T = len(area_rng), len(limits), len(thr)
    assert prop_off.dtype == torch.int64 and gt_off.dtype == torch.int64 and item_off.dtype == torch.int64
    assert prop_box.dtype == torch.float32 and gt_box.dtype == torch.float32 and gt_area.dtype == torch.float32
    assert n_img >= 0 and prop_off.shape == (n_img + 1,) and gt_off.shape == (n_img + 1,) and item_off.dim() == 1
    assert prop_box.shape == (P, 4) and gt_box.shape == (G, 4) and gt_area.shape == (G,)
    for t in (prop_off, prop_box, gt_off, gt_box, gt_area, item_off):
        assert t.is_contiguous()
    dev = prop_box.device
    assert item_off.numel() >= 1
    big_p = big_g = 0
    if n_img > 0 and (check_offsets or max_boxes is None or max_props is None):          # one device-to-host copy
        dp, dg = prop_off.diff(), gt_off.diff()
        di_min = item_off.diff().min() if item_off.numel() > 1 else item_off.new_zeros(())
        v = torch.stack([dp.min(), dg.min(), di_min, prop_off[0], gt_off[0], item_off[0], prop_off[-1], gt_off[-1], dp.max(),
                         dg.max()]).tolist()
        if check_offsets and (min(v[:3]) < 0 or any(v[3:6]) or v[6] > P or v[7] > G):
            raise ValueError("box_proposal_ar: offsets must start at 0, never decrease and end inside their arrays")
        big_p, big_g = int(v[8]), int(v[9])
    if max_boxes is None:
        max_boxes = big_g
    if max_props is None:
        max_props = big_p if (not limits or min(limits) <= 0) else min(big_p, max(limits))
    if overlap is None:
        overlap = torch.empty(int(item_off[-1].item()), device=dev, dtype=torch.float32)
    if match_gt is None:
        match_gt = torch.empty(overlap.numel(), device=dev, dtype=torch.int32)
    if match_box is None:
        match_box = torch.empty(overlap.numel(), device=dev, dtype=torch.int32)
    assert overlap.dtype == torch.float32 and match_gt.dtype == torch.int32 and match_box.dtype == torch.int32
    assert overlap.dim() == 1 and match_gt.shape == overlap.shape and match_box.shape == overlap.shape
    assert overlap.is_contiguous() and match_gt.is_contiguous() and match_box.is_contiguous()
    cnt_yes = torch.empty(max(L, 1), max(A, 1), max(T, 1), device=dev, dtype=torch.int64)
    status = torch.empty(1, device=dev, dtype=torch.int32)
    nbytes = lib.sw_box_proposal_ar_workspace_bytes(n_img, int(max_boxes), int(max_props))
    assert nbytes >= 0, "sw_box_proposal_ar_workspace_bytes"
    ws, ws_p = _workspace256(nbytes, dev) if nbytes else (None, None)
    check(lib.sw_box_proposal_ar(n_img, _p(prop_off), _p(prop_box), P, _p(gt_off), _p(gt_box), _p(gt_area), G, A,
                                 _floats([v for r in area_rng for v in r], max(2 * A, 1)), L,
                                 (ctypes.c_int32 * max(L, 1))(*limits), T, _floats(thr, max(T, 1)), _p(item_off), item_off.numel(),
                                 overlap.numel(), _p(overlap), _p(match_gt), _p(match_box), _p(cnt_yes), ws_p, nbytes, int(max_boxes),
                                 int(max_props), _p(status), _stream()), "sw_box_proposal_ar")
    return overlap, match_gt, match_box, cnt_yes, status


# ================================================================================================ JPEG reader (csrc/jpeg.hip)
def jpeg_error(code):
    """the host code's reason for a probe / entropy-decode return code"""
    return lib.sw_jpeg_strerror(int(code)).decode()


def jpeg_probe(data):
    """sw_jpeg_probe over a contiguous uint8 numpy array (HOST code, no GPU).  -> (code, JpegInfo): 1 covered, 0 left to Pillow,
    negative malformed (-2: not a JPEG at all)"""
    from ._lib import JpegInfo
    info = JpegInfo()
    return lib.sw_jpeg_probe(ctypes.c_void_p(data.ctypes.data), data.size, ctypes.byref(info)), info


def jpeg_entropy_decode(data, info, coef_addr, qtab_addr):
    """sw_jpeg_entropy_decode (HOST code; ctypes drops the GIL for its duration): info.coef_bytes bytes of int16 coefficients to
    coef_addr, 512 bytes of tables to qtab_addr, both host addresses.  -> the return code"""
    return lib.sw_jpeg_entropy_decode(ctypes.c_void_p(data.ctypes.data), data.size, ctypes.byref(info), ctypes.c_void_p(coef_addr),
                                      ctypes.c_void_p(qtab_addr))


def jpeg_workspace_bytes(infos):
    """bytes of planes sw_jpeg_decode_batch writes for these images; infos: a ctypes array of JpegInfo"""
    n = lib.sw_jpeg_workspace_bytes(len(infos), infos)
    if n < 0:
        raise ValueError("sw_jpeg_workspace_bytes: an info does not describe a covered image")
    return n


def jpeg_describe_batch(infos, outs, bgr, descs_addr):
    """fill len(infos) sw_jpeg_desc records at the host address descs_addr (sw_jpeg_describe_batch).  outs: (3, H, W) uint8 device
    tensors.  -> (total_blocks, total_quads)"""
    from ._lib import JpegDesc
    n = len(infos)
    for o, f in zip(outs, infos):
        _need_gpu(o)
        assert o.dtype == torch.uint8 and tuple(o.shape) == (3, f.height, f.width) and o.is_contiguous(), "out: contiguous (3, H, W) uint8"
    ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    tb, tq = ctypes.c_long(), ctypes.c_long()
    check(lib.sw_jpeg_describe_batch(n, infos, ptrs, int(bool(bgr)), ctypes.cast(descs_addr, ctypes.POINTER(JpegDesc)),
                                     ctypes.byref(tb), ctypes.byref(tq)), "sw_jpeg_describe_batch")
    return tb.value, tq.value


def jpeg_decode_batch(n, descs_addr, total_blocks, total_quads, coef_addr, qtab_addr, workspace_addr):
    """the two launches of sw_jpeg_decode_batch on the current stream; every address is a device address"""
    check(lib.sw_jpeg_decode_batch(n, ctypes.c_void_p(descs_addr), total_blocks, total_quads, ctypes.c_void_p(coef_addr),
                                   ctypes.c_void_p(qtab_addr), ctypes.c_void_p(workspace_addr), _stream()), "sw_jpeg_decode_batch")
