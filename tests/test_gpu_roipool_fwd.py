"""The ROIPool forward (csrc/roipool.hip: sw_roi_pool_fwd, launch_fwd_tasks, roi_fwd_dispatch, launch_fwd_sparse and the six kernel
forms behind them) through ops.roi_pool_fwd, at every edge of its dispatch, against the C oracle (oracle.oicr_oracle.roi_pool_fwd).

Every case: asserts the form the dispatch must take (roipool_ref.fwd_plan), prefills out, argmax and an oversized workspace with a
byte pattern, and compares EVERY bin of every channel of every ROI with the oracle: argmax exactly (through ops.argmax_to_int32),
values bit for bit (oracle value * float32(row_scale + add), rounded to the output type; the sign of a zero and of a NaN included).
One deviation is the library's design and is asserted as such: the packed-key forms (FwdPlan.key: every bf16 form but the gather
one) order values by a 16-bit key in which -0.0 and +0.0 are one key, so that the earlier pixel wins as under the reference's '>',
and a bin won by a -0.0 pixel comes out as +0.0 (key16_of in roipool.hip).  No tolerance: the forward copies values.  Then: nothing outside [R][C * PH * PW] of out / argmax has changed (pitch gap, rows past R), nothing past the declared
workspace bytes has changed, and the declared bytes have changed exactly when the plan says "tasks" — the one form that can be
observed from outside the library.  The cases and what each is built to reach are in roipool_ref.py; tests/test_roipool_ref_cpu.py
shows that each has its property.

Sharpness, checked once on MI355X with changed copies of the library (each by reading never forms an address out of range):
  BandGeom::owner without the cap (plane-band and sparse call sites)   red: classes sparse_band_ / plane_band_H_multiple_of_S,
                                                                         thresholds R16384, PW2_ws, ws_absent, band_W, band_R, nimg65,
                                                                         declined_tasks
  band_geometry's halo one row smaller                                   red: thresholds bands17 (the workspace is written: 16 bands, the
                                                                         task form) and declined_plane_band (the band form takes it).
                                                                         Values inside a band stay right: rows past a band's slab are read
                                                                         from global memory, the halo is a matter of speed
  key16_of without its -0.0 rule                                         red: 186 cases, the signed_zero channel of every values case first
  for_my_rois stepping 9 * n_zsplit                                      red: chunks sparse_whole_rounds_R1025 / _R2177, sparse_band_rounds_R1025
  for_my_rois stepping 7 * n_zsplit                                      green, and no case can see it: every block is still visited, one in
                                                                         seven twice, and a ROI listed twice writes the same bins twice
  the sparse whole form one row early                                    red: thresholds band_H_past_lds (the launch is rejected)
  roi_level_class without the level cap                                  not run: the class then indexes past s_start and the task form's
                                                                         histogram cells
A kernel trace of one case per form showed the kernels FwdPlan.kernels names and no other roi_pool_* kernel (the whole and band forms of
the sparse and plane kernels are template arguments of one name; the workspace check above is what tells the task form apart)."""
import functools

import numpy as np
import pytest
import torch

import roipool_ref as RR
from oracle import oicr_oracle as O

pytestmark = pytest.mark.gpu

TDT = {"bf16": torch.bfloat16, "f32": torch.float32}
FILL = 0xA5
EXTRA_ROWS = 2
WS_TAIL = 272


@pytest.fixture(scope="module")
def ops():
    import sos_wsod_amd  # noqa: F401
    import sos_wsod_amd.ops as ops
    assert torch.cuda.is_available()
    return ops


def _ids(cases):
    return [c.name.split("/", 1)[1] for c in cases]


def _bytes(t):
    return t.contiguous().view(torch.uint8)


@functools.lru_cache(maxsize=8)
def _reference(group, index):
    """(feat NCHW float32, oracle values, oracle argmax) of a case, computed once for the tests that share it"""
    case = RR.fwd_cases(group)[index]
    feat = case.feat()
    if case.R == 0:
        return feat, None, None
    out, arg = O.roi_pool_fwd(feat, case.rois, RR.SCALE, case.PH, case.PW)
    return feat, out, arg


class _Call:
    """the device tensors of a case: feat at its byte offset, out / argmax with pitch gap and rows past R, the oversized workspace"""

    def __init__(self, ops, case, feat, argmax_bits=None):
        self.ops, self.case = ops, case
        nimg, H, W, C = case.shape
        tdt = TDT[case.dtype]
        es = 2 if case.dtype == "bf16" else 4
        n = nimg * H * W * C
        off = case.feat_offset // es
        buf = torch.zeros(n + 16, dtype=tdt, device="cuda")
        self.feat = buf[off:off + n].view(nimg, H, W, C)
        self.feat.copy_(torch.from_numpy(feat).permute(0, 2, 3, 1).to(tdt))
        assert self.feat.data_ptr() % 16 == case.feat_offset
        self.bits = argmax_bits or case.argmax_bits
        R, row = case.R, C * case.PH * case.PW
        self.R, self.row = R, row
        ld = row + case.pad
        rows = R + EXTRA_ROWS
        adt = torch.int16 if self.bits == 16 else torch.int32
        self.out_full = torch.empty(rows * max(ld, row), dtype=tdt, device="cuda")
        self.arg_full = torch.empty(rows * max(ld, row), dtype=adt, device="cuda")
        self.out_full.view(torch.uint8).fill_(FILL)
        self.arg_full.view(torch.uint8).fill_(FILL)
        self.out = self.out_full.as_strided((R, row), (ld, 1))
        self.arg = self.arg_full.as_strided((R, row), (ld, 1))
        self.ld = ld
        self.rois = torch.from_numpy(case.rois).cuda()
        rs, self.add = case.scales()
        self.rs_host = rs
        self.row_scale = None if rs is None else torch.from_numpy(rs).cuda()
        self.ws_full = self.ws = None
        self.need = 0
        if case.workspace is not None and R > 0:
            self.need = need = int(ops.roi_pool_fwd_workspace(nimg, R, case.PH, case.PW, "cuda").numel())
            assert need == RR.fwd_workspace_bytes(nimg, R, case.PH, case.PW)
            self.ws_full = torch.full((need + WS_TAIL,), FILL, dtype=torch.uint8, device="cuda")
            lo = 8 if case.workspace == "misaligned" else 0
            self.declared = need - 1 if case.workspace == "short" else need
            self.ws = self.ws_full[lo:lo + self.declared]
            self.ws_lo = lo
        self.before = (self.out_full.clone(), self.arg_full.clone())

    def launch(self):
        c = self.case
        self.ops.roi_pool_fwd(self.feat, self.rois, self.out, self.arg, RR.SCALE, c.PH, c.PW, row_scale=self.row_scale,
                              row_scale_add=self.add, workspace=self.ws)
        torch.cuda.synchronize()

    def assert_outside_untouched(self, written):
        """nothing but [R][row] of out / argmax differs from the fill (written = False: nothing at all)"""
        for full, before in zip((self.out_full, self.arg_full), self.before):
            now = full.clone()
            if written:
                now.as_strided((self.R, self.row), (self.ld, 1)).copy_(before.as_strided((self.R, self.row), (self.ld, 1)))
            assert torch.equal(_bytes(now), _bytes(before)), "bytes outside [R][C * PH * PW] were written"

    def assert_workspace(self, tasks):
        if self.ws_full is None:
            return
        ws = self.ws_full.cpu()
        end = self.ws_lo + self.declared
        assert bool((ws[end:] == FILL).all()) and bool((ws[:self.ws_lo] == FILL).all()), "bytes outside the declared workspace were written"
        changed = bool((ws[self.ws_lo:end] != FILL).any())
        assert changed == tasks, f"the declared workspace {'was not' if tasks else 'was'} written: the call did {'not ' if tasks else ''}take the prepared-task form"

    def results(self):
        """(values as float32 (R, C, PH, PW), argmax as int32 (R, C, PH, PW))"""
        c = self.case
        shape = (self.R, c.shape[3], c.PH, c.PW)
        arg = self.ops.argmax_to_int32(self.arg.contiguous()).cpu().numpy().reshape(shape)
        return self.out.contiguous().float().cpu().numpy().reshape(shape), arg

    def expected_values(self, ref_out):
        want = torch.from_numpy(ref_out)
        if self.rs_host is not None:
            want = want * torch.from_numpy(RR.row_multiplier(self.rs_host, self.add, self.R)).view(-1, 1, 1, 1)
        return want.to(TDT[self.case.dtype]).float().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _compare(case, plan, call, ref_out, ref_arg):
    got, got_arg = call.results()
    bad = np.argwhere(got_arg != ref_arg)
    assert len(bad) == 0, (f"{case.name}: argmax differs in {len(bad)} of {ref_arg.size} bins; first (roi, channel, ph, pw) {bad[:4].tolist()}: "
                           f"got {[int(got_arg[tuple(b)]) for b in bad[:4]]}, oracle {[int(ref_arg[tuple(b)]) for b in bad[:4]]}, "
                           f"rois {[case.rois[b[0]].tolist() for b in bad[:2]]}")
    want = call.expected_values(ref_out)
    got_bits, want_bits = _bits(got), _bits(want)
    same = got_bits == want_bits
    if plan.key:                                   # a bin won by a -0.0 pixel: +0.0, and nothing else, from the packed-key forms
        same |= (want_bits == 0x80000000) & (got_bits == 0)
    bad = np.argwhere(~same)
    assert len(bad) == 0, (f"{case.name}: values differ in {len(bad)} of {want.size} bins; first (roi, channel, ph, pw) {bad[:4].tolist()}: "
                           f"got {[float(got[tuple(b)]) for b in bad[:4]]}, want {[float(want[tuple(b)]) for b in bad[:4]]}")


def _run(ops, group, index):
    """everything a case is checked for"""
    from sos_wsod_amd._lib import HipKernelError
    case = RR.fwd_cases(group)[index]
    plan = RR.check_fwd_plan(case)
    feat, ref_out, ref_arg = _reference(group, index)
    call = _Call(ops, case, feat)
    if case.form == "refused":
        with pytest.raises(HipKernelError, match=f"sw_roi_pool_fwd failed with code {case.code}$"):
            call.launch()
        torch.cuda.synchronize()
        call.assert_outside_untouched(written=False)
        call.assert_workspace(tasks=False)
        return call
    call.launch()
    if case.form == "none":
        call.assert_outside_untouched(written=False)
        return call
    _compare(case, plan, call, ref_out, ref_arg)
    call.assert_outside_untouched(written=True)
    call.assert_workspace(tasks=plan.form == "tasks")
    return call


def _group_test(group):
    cases = RR.fwd_cases(group)

    @pytest.mark.parametrize("index", range(len(cases)), ids=_ids(cases))
    def test(ops, index):
        _run(ops, group, index)
    return test


test_forms = _group_test("forms")
test_thresholds = _group_test("thresholds")
test_chunks = _group_test("chunks")
test_classes = _group_test("classes")
test_values = _group_test("values")
test_slabs = _group_test("slabs")
test_untouched = _group_test("untouched")


_FORM_FIRST = [i for i, c in enumerate(RR.fwd_cases("forms")) if c.argmax_bits == 16]


@pytest.mark.parametrize("index", _FORM_FIRST, ids=[_ids(RR.fwd_cases("forms"))[i] for i in _FORM_FIRST])
def test_two_launches_and_both_index_widths_agree(ops, index):
    """one case per form and channel width: two launches give the same bits; 16- and 32-bit argmax decode to the same indices"""
    case = RR.fwd_cases("forms")[index]
    RR.check_fwd_plan(case)
    feat, ref_out, ref_arg = _reference("forms", index)
    runs = []
    for bits in (16, 16, 32):
        call = _Call(ops, case, feat, argmax_bits=bits)
        call.launch()
        runs.append((call.out.contiguous().cpu(), call.arg.contiguous().cpu(), call.results()[1]))
    assert torch.equal(_bytes(runs[0][0]), _bytes(runs[1][0])) and torch.equal(runs[0][1], runs[1][1]), "two launches differ"
    assert torch.equal(_bytes(runs[0][0]), _bytes(runs[2][0])), "values differ between 16- and 32-bit argmax"
    assert np.array_equal(runs[0][2], runs[2][2]) and np.array_equal(runs[2][2], ref_arg), "decoded indices differ between 16- and 32-bit argmax"
