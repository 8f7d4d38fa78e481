"""The ROIPool backward (csrc/roipool.hip: roi_bwd_dispatch, roi_pool_bwd_fx_kernel, roi_pool_bwd_kernel) through
ops.roi_pool_bwd, at every edge of its dispatch, against the float64 scatter-add of tests/roipool_ref.py.

Every case: asserts the plan the dispatch must take (roipool_ref.bwd_plan), prefills dfeat and guard bands around it with NaN,
compares EVERY element with the reference within the per-element bar derived in roipool_ref.bwd_bar (printed: largest
error / bar), and checks that the guards and the pitch gaps of the inputs are as they were.  On the fixed-point path two
launches must give equal bits, and so must spatial_scale = 0 and the forward's scale.  The cases and what each is built to
reach are in roipool_ref.py; tests/test_roipool_ref_cpu.py shows that each has its property."""
import functools

import numpy as np
import pytest
import torch

import roipool_ref as RR

pytestmark = pytest.mark.gpu

GUARD = 64
TDT = {"bf16": torch.bfloat16, "f32": torch.float32}
DTYPES = ["bf16", "f32"]


@pytest.fixture(scope="module")
def ops():
    import sos_wsod_amd  # noqa: F401
    import sos_wsod_amd.ops as ops
    assert torch.cuda.is_available()
    return ops


@functools.lru_cache(maxsize=4)
def _built(builder, *args):
    """a case and its reference, built once for the tests that share it"""
    case = getattr(RR, builder)(*args)
    return case, case.reference()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class _Call:
    """the device tensors of a case, laid out with its pitch, gaps and offset"""

    def __init__(self, ops, case):
        self.ops, self.case = ops, case
        nimg, H, W, C = case.shape
        R, row = case.R, C * case.PH * case.PW
        ld = row + case.pad
        tdt = TDT[case.dtype]
        d = torch.full((case.offset + R * ld,), float("nan"), dtype=tdt)              # gaps of dout: NaN
        d[case.offset:].view(R, ld)[:, :row] = torch.from_numpy(case.dout.reshape(R, row)).to(tdt)
        a = np.zeros((R, ld), np.int32)                                                # gaps of argmax: a valid pixel
        a[:, :row] = case.argmax.reshape(R, row)
        if case.argmax_bits == 16:
            a = np.where(a < 0, 0xFFFF, a).astype(np.uint16).view(np.int16)
        self.d_host, self.a_host = d, torch.from_numpy(a)
        self.d_dev, self.a_dev = d.cuda(), self.a_host.cuda()
        self.dout = self.d_dev[case.offset:].view(R, ld)[:, :row]
        self.arg = self.a_dev[:, :row]
        self.rois = torch.from_numpy(case.rois).cuda()
        self.row_scale = None if case.row_scale is None else torch.from_numpy(case.row_scale).cuda()
        self.relu = None if case.relu_ref is None else torch.from_numpy(case.relu_ref).to(tdt).cuda()
        self.absmax = ops.absmax(self.dout.contiguous()) if case.has_absmax else None
        self.n = nimg * H * W * C

    def launch(self, spatial_scale=0.0):
        case = self.case
        full = torch.full((self.n + 2 * GUARD,), float("nan"), device="cuda", dtype=TDT[case.dtype])
        dfeat = full[GUARD:GUARD + self.n].view(case.shape)
        self.ops.roi_pool_bwd(self.dout, self.arg, self.rois, dfeat, case.PH, case.PW, row_scale=self.row_scale,
                              row_scale_add=case.add, relu_ref=self.relu, dout_absmax=self.absmax, spatial_scale=spatial_scale)
        torch.cuda.synchronize()
        assert torch.isnan(full[:GUARD]).all() and torch.isnan(full[GUARD + self.n:]).all(), "guard band written"
        return dfeat.cpu()

    def inputs_untouched(self):
        assert torch.equal(_bits(self.d_dev.cpu()), _bits(self.d_host)) and torch.equal(self.a_dev.cpu(), self.a_host)


def _assert_plan(case):
    p = case.plan()
    assert (p.path, p.CB) == (case.path, case.CB), (case.name, p)
    if case.path == "fx":
        assert (p.nsplit, p.accmode) == (case.nsplit, case.accmode), (case.name, p)


def _assert_within_bar(case, br, got, label=""):
    bar = case.bar(br)
    err = np.abs(got.double().numpy() - br.ref)
    ratio = err / bar
    bad = ~(err <= bar)                                                                # a NaN left in dfeat is bad too
    print(f"\n{case.name}{label}: largest error / bar {np.nanmax(ratio):.4f} over {ratio.size} elements, {int(bad.sum())} outside")
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio))), ratio.shape)
        raise AssertionError(f"{case.name}{label}: {int(bad.sum())} of {ratio.size} elements outside their bar; worst at "
                             f"(image, row, column, channel) {i[0], i[1], i[2], i[3]}: got {float(got[i])!r}, reference {br.ref[i]!r}, "
                             f"bar {bar[i]:.3e}, terms {int(br.n[i])}")


def _run(ops, case, br, primary_scale=0.0, both_scales=True):
    """everything a case is checked for; returns the primary launch's result"""
    _assert_plan(case)
    call = _Call(ops, case)
    got = call.launch(primary_scale)
    _assert_within_bar(case, br, got, f" [scale {primary_scale:g}]")
    if case.path == "fx":
        assert torch.equal(_bits(call.launch(primary_scale)), _bits(got)), "two launches differ"
        if case.scale and both_scales:
            other = case.scale if primary_scale == 0.0 else 0.0
            assert torch.equal(_bits(call.launch(other)), _bits(got)), "spatial_scale = 0 and the forward's scale differ"
    call.inputs_untouched()
    return got


# ---------------------------------------------------------------------------------------------- 1. last-bin overshoot
@pytest.mark.parametrize("scale", ["zero", "forward"])
@pytest.mark.parametrize("argmax_bits", [16, 32])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(RR.OVERSHOOT_MAPS))
def test_rois_whose_last_bin_reaches_the_row_after_their_end(ops, name, dtype, argmax_bits, scale):
    """ROI heights 57, 114 and 121: the forward's last bin takes in row re + 1, and that row starts (or lies in) the map's
    second pixel range.  A ROI filter that trusts [rs, re] drops those gradients when it is given the forward's scale ("forward",
    which also asks for the bits of scale 0); with scale 0 every ROI is streamed ("zero")."""
    case, br = _built("overshoot_case", name, dtype, argmax_bits)
    _run(ops, case, br, 0.0 if scale == "zero" else case.scale, both_scales=scale == "forward")


# ---------------------------------------------------------------------------------------------- 2. range edges
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nsplit", sorted(RR.RANGE_MAPS))
def test_pixel_range_edges(ops, nsplit, dtype):
    """1, 2, 5 and 16 pixel ranges per plane; argmax at p0 - 1, p0, p1 - 1 of every range and at the map's last pixel"""
    case, br = _built("range_edge_case", nsplit, dtype)
    _run(ops, case, br)


def test_map_beyond_sixteen_ranges_is_refused(ops):
    from sos_wsod_amd._lib import HipKernelError
    H, W, C, R = 240, 321, 4, 2
    assert RR.bwd_plan("bf16", 32, 1, H, W, C, 2, 2, R, 0, True, True).path == "refused"
    dout = torch.ones(R, C * 4, device="cuda", dtype=torch.bfloat16)
    arg = torch.zeros(R, C * 4, device="cuda", dtype=torch.int32)
    dfeat = torch.zeros(1, H, W, C, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(HipKernelError, match="sw_roi_pool_bwd failed with code -6"):
        ops.roi_pool_bwd(dout, arg, torch.zeros(R, 5, device="cuda"), dfeat, 2, 2)
    torch.cuda.synchronize()
    assert not dfeat.any()


# ---------------------------------------------------------------------------------------------- 3. pooled sizes
@pytest.mark.parametrize("dtype,C", [("bf16", 4), ("f32", 4), ("bf16", 1024)])
@pytest.mark.parametrize("P", RR.POOLED, ids=lambda p: f"{p[0]}x{p[1]}")
def test_pooled_sizes_and_slab_widths(ops, P, dtype, C):
    """pooled sizes from 1 x 1 (a lane's four elements are four channels) to 14 x 14, slabs of 4 and of 8 channels"""
    case, br = _built("pooled_case", P[0], P[1], dtype, C)
    _run(ops, case, br)


# ---------------------------------------------------------------------------------------------- 4. chunks and tails
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("R", RR.CHUNK_R)
def test_roi_counts_around_the_chunk_and_the_step(ops, R, relu):
    case, br = _built("chunk_case", R, relu)
    got = _run(ops, case, br)
    assert not got[2].any()                                                            # the image without ROIs


# ---------------------------------------------------------------------------------------------- 5. accumulator sizing
@pytest.mark.parametrize("absmax", [1 - 2.0 ** -8, 1.0])
@pytest.mark.parametrize("R", [1023, 1024, 1025])
def test_full_accumulators_bf16(ops, R, absmax):
    """8 x 8 bins of R ROIs, every term +absmax, on one pixel of every channel: the hi word as full as the sizing allows"""
    case, br = _built("pile_case", 8, R, absmax)
    got = _run(ops, case, br)
    assert float(got[0, 1, 1, 0]) == float(torch.tensor(64.0 * R * absmax).to(torch.bfloat16))      # an exact sum, rounded once


@pytest.mark.parametrize("absmax", [1 - 2.0 ** -24, 1.0])
def test_full_accumulators_f32(ops, absmax):
    case, br = _built("pile_case", 8, 1024, absmax, "f32")
    _run(ops, case, br)


def test_bf16_takes_64_bit_accumulators_at_2_to_22_terms(ops):
    case = RR.pile_case(16, 16384, 1 - 2.0 ** -8)
    assert case.accmode == 0 and case.R * 256 == 1 << 22
    _run(ops, case, case.reference())


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients_over_many_decades_leave_no_dead_zone(ops, dtype):
    case, br = _built("lognormal_case", dtype)
    got = _run(ops, case, br).double().numpy()
    seen = np.abs(br.ref) > 1e-6 * np.abs(br.ref).max()
    assert seen.sum() > seen.size // 2 and np.all(got[seen] != 0)


# ---------------------------------------------------------------------------------------------- 6. scales and masks
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["negative", "decades", "zero"])
def test_row_scales_and_relu_masks(ops, kind, dtype):
    """negative row scales, row scales over 30 decades, row_scale + add == 0 everywhere; a mask with NaN, -0.0 and negatives"""
    case, br = _built("scale_case", kind, dtype)
    got = _run(ops, case, br)
    assert not got[~(torch.from_numpy(case.relu_ref) > 0)].any()
    if kind == "zero":
        assert not got.any()


# ---------------------------------------------------------------------------------------------- 7. poison
@pytest.mark.parametrize("path", ["fx", "float"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", RR.POISONS)
def test_non_finite_inputs_reach_the_gradient(ops, kind, dtype, path):
    """a NaN or Inf in dout or in row_scale: the fixed-point path writes NaN over the image the ROI belongs to, the float
    atomics carry the value to the element it reaches; never a finite number in its place"""
    case, br = _built("poison_case", kind, dtype, path == "fx")
    _assert_plan(case)
    call = _Call(ops, case)
    got = call.launch()
    bad = ~np.isfinite(br.ref)
    assert bad[0].any() and not bad[1].any()
    if path == "fx":
        assert torch.isnan(got[0]).all()
    else:
        g = got.double().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(br.ref)) and np.array_equal(g[bad & ~np.isnan(br.ref)], br.ref[bad & ~np.isnan(br.ref)])
        fin = RR.BwdRef(br.ref[1:], br.n[1:], br.S[1:], br.tmax[1:])
        bar = RR.bwd_bar(case.plan(), fin, dtype)
        assert np.all(np.abs(g[1:] - fin.ref) <= bar)
    call.inputs_untouched()


# ---------------------------------------------------------------------------------------------- 8. float-atomic fallback
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", RR.FALLBACKS)
def test_float_atomic_fallback(ops, kind, dtype):
    """no absmax, a pitch that is no multiple of 4, channel counts 6 and 2, a dout that starts one element in"""
    case, br = _built("fallback_case", kind, dtype)
    assert case.plan().path == "float"
    _run(ops, case, br)


@pytest.mark.parametrize("args", [(7, 7, "bf16", 1024), (1, 1, "f32", 4), (14, 14, "bf16", 4)], ids=str)
def test_float_atomic_slab_widths(ops, args):
    case, br = _built("pooled_case", *args, False)
    assert case.plan().path == "float"
    _run(ops, case, br)


# ---------------------------------------------------------------------------------------------- 9. pitch gaps
@pytest.mark.parametrize("path", ["fx", "float"])
@pytest.mark.parametrize("argmax_bits", [16, 32])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pitch_gaps_are_not_read(ops, dtype, argmax_bits, path):
    """the gaps of dout hold NaN and those of argmax a valid pixel: either would show in dfeat"""
    case, br = _built("gap_case", dtype, argmax_bits, path)
    assert case.pad > 0
    _run(ops, case, br)
