"""CPU: the float64 restatements of tests/losses_ref.py against float64 torch autograd of the reference's own expressions and against
the oracles (oracle.frcnn_oracle.rpn_losses, oracle.semisup_oracle.focal_loss), the input conditions the GPU edge tests of
tests/test_gpu_loss_kernels.py rely on (distance of every foreground box residual from the kink of the L1 loss, exact ties at the
selection threshold, the launch edges the case tables are meant to hold), and the tolerance table losses_ref.E32 (recomputed here;
`python tests/test_losses_ref_cpu.py` prints a fresh table)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import frcnn_oracle as FO  # noqa: E402
from oracle import oicr_oracle as O  # noqa: E402
from oracle import semisup_oracle as SO  # noqa: E402
import losses_ref as L  # noqa: E402

PIN64 = 1e-12           # float64 restatement against float64 autograd of the same expression
PIN = 1e-3              # a wrong restatement is off by O(1); float32 against float64 of these formulas stays far below this


def _note(tab, kind, regime, f32, f64):
    e = L.rel_err(f32, f64)
    tab[(kind, regime)] = max(tab.get((kind, regime), 0.0), e)
    return e


def _rpn_args(i):
    return i["logits"], i["deltas"], i["labels"], i["anchors"], i["matched"], i["weights"], i["inv_norm"]


def fresh_table():
    """-> (e32 table, per-case records) over every case of the GPU tests"""
    tab, rec = {}, {"rpn": {}}
    for c in L.RPN_CASES:
        i = L.rpn_inputs(c)
        ref, f32 = L.rpn_loss_ref(*_rpn_args(i)), L.rpn_loss_f32(*_rpn_args(i))
        for k in ("loss_cls", "loss_loc", "dlogits"):
            _note(tab, "rpn." + k, c["w"], f32[k], ref[k])
        rec["rpn"][c["id"]] = dict(ref=ref, f32=f32, inp=i)
    for c in L.FOCAL_CASES:
        x, t = L.focal_inputs(c)
        l64, g64 = L.focal_ref(x, t, c["gamma"]); l32, g32 = L.focal_f32(x, t, c["gamma"])
        reg = L.focal_tol_regime(c)
        _note(tab, "focal.loss", reg, l32, l64); _note(tab, "focal.dlogits", reg, g32, g64)
    for c in L.DETLOSS_CASES:
        inp = L.detloss_inputs(c)
        for box_type, gamma in L.DETLOSS_TYPES:
            a = (inp, c["rpn_bs"], box_type, c["K"], gamma, box_type)
            r64, r32 = L.det_loss_ref(*a), L.det_loss_f32(*a)
            assert (np.isnan(r64) == np.isnan(r32)).all(), (c["id"], box_type, gamma)
            _note(tab, "detloss.out", "all", np.nan_to_num(r32), np.nan_to_num(r64))
    for c in L.SCORES_BWD_CASES:
        x, g = L.scores_bwd_inputs(c)
        (c64, d64), (c32, d32) = L.wsddn_scores_bwd_ref(x, c["K"], g), L.wsddn_scores_bwd_f32(x, c["K"], g)
        reg = f"amp{c['amp']:g}"
        _note(tab, "scores_bwd.dC", reg, c32, c64); _note(tab, "scores_bwd.dD", reg, d32, d64)
    return tab, rec


@pytest.fixture(scope="module")
def fresh():
    return fresh_table()


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    m = float(np.abs(b).max()) if b.size else 0.0
    d = float(np.abs(a - b).max()) if b.size else 0.0
    return 0.0 if d == 0.0 else d / m


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("c", [c for c in L.RPN_CASES if c["N"] * c["A"] < 70000], ids=lambda c: c["id"])
def test_rpn_loss_ref_equals_float64_autograd_of_the_reference_expression(c):
    """F.binary_cross_entropy_with_logits over label >= 0 + L1 on get_deltas over label == 1, both x inv_norm, in float64"""
    i = L.rpn_inputs(c)
    ref = L.rpn_loss_ref(*_rpn_args(i))
    x = torch.from_numpy(i["logits"]).double().requires_grad_(True); d = torch.from_numpy(i["deltas"]).double().requires_grad_(True)
    lab = torch.from_numpy(i["labels"].astype(np.int64))
    A = i["anchors"].shape[0]
    valid, fg = lab >= 0, torch.nonzero(lab == 1)[:, 0]
    s = float(i["inv_norm"])
    cls = F.binary_cross_entropy_with_logits(x[valid], (lab[valid] == 1).double(), reduction="sum") * s
    tgt = O.get_deltas(torch.from_numpy(i["anchors"]).double()[fg % A], torch.from_numpy(i["matched"]).double()[fg], i["weights"])
    loc = (d[fg] - tgt).abs().sum() * s
    (cls + loc).backward()
    assert _rel(ref["loss_cls"], cls.item()) <= PIN64 and _rel(ref["loss_loc"], loc.item()) <= PIN64
    assert _rel(ref["dlogits"], x.grad.numpy()) <= PIN64
    assert np.array_equal(ref["ddeltas"], d.grad.numpy())                       # signs times one factor: exact
    part = i["labels"] >= 0
    assert np.all(ref["dlogits"][~part] == 0) and np.all(ref["ddeltas"][i["labels"] != 1] == 0)
    if c["labels"] == "ignore":
        assert ref["loss_cls"] == 0.0 and ref["loss_loc"] == 0.0


@pytest.mark.parametrize("c", L.FOCAL_CASES, ids=lambda c: c["id"])
def test_focal_ref_equals_float64_autograd_of_the_reference_expression(c):
    """((1 - exp(-ce)) ** gamma * ce).sum() / N with ce = F.cross_entropy(reduction="none") in float64"""
    x, t = L.focal_inputs(c)
    loss, g = L.focal_ref(x, t, c["gamma"])
    xt = torch.from_numpy(x).double().requires_grad_(True)
    ce = F.cross_entropy(xt, torch.from_numpy(t).long(), reduction="none")
    lt = ((1 - torch.exp(-ce)) ** c["gamma"] * ce).sum() / x.shape[0]
    lt.backward()
    assert _rel(loss, lt.item()) <= PIN64, (loss, lt.item())
    assert _rel(g, xt.grad.numpy()) <= PIN64
    if c["C"] == 1:
        assert loss == 0.0 and not g.any()


@pytest.mark.parametrize("c", L.SCORES_BWD_CASES, ids=lambda c: c["id"])
def test_scores_bwd_ref_equals_float64_autograd_of_the_reference_expression(c):
    """softmax(C, 1) * softmax(D, 0) contracted with g"""
    x, g = L.scores_bwd_inputs(c)
    K = c["K"]
    dC, dD = L.wsddn_scores_bwd_ref(x, K, g)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    (F.softmax(xt[:, :K], 1) * F.softmax(xt[:, K:], 0) * torch.from_numpy(g).double()).sum().backward()
    assert _rel(dC, xt.grad[:, :K].numpy()) <= PIN64 and _rel(dD, xt.grad[:, K:].numpy()) <= PIN64


def test_rpn_loss_ref_agrees_with_the_oracle():
    """oracle.frcnn_oracle.rpn_losses (float32 torch, weights (1, 1, 1, 1)) on the shape of test_gpu_stage3's kernel test"""
    c = dict(N=2, A=417, labels="mixed", w="w1")
    i = L.rpn_inputs(c)
    N, A = c["N"], c["A"]
    lt = torch.from_numpy(i["logits"]).view(N, A).clone().requires_grad_(True)
    dt = torch.from_numpy(i["deltas"]).view(N, A, 4).clone().requires_grad_(True)
    r = FO.rpn_losses(i["anchors"], [lt], [dt], [i["labels"].reshape(N, A)[k].astype(np.int64) for k in range(N)],
                      [i["matched"].reshape(N, A, 4)[k] for k in range(N)], batch_size=256)
    (r["loss_rpn_cls"] + r["loss_rpn_loc"]).backward()
    ref = L.rpn_loss_ref(*_rpn_args(i))
    assert L.rel_err(r["loss_rpn_cls"].item(), ref["loss_cls"]) <= 1e-5 and L.rel_err(r["loss_rpn_loc"].item(), ref["loss_loc"]) <= 1e-5
    assert L.rel_err(lt.grad.numpy().reshape(-1), ref["dlogits"]) <= 1e-5
    assert L.rel_err(dt.grad.numpy().reshape(-1, 4), ref["ddeltas"]) <= 1e-6


@pytest.mark.parametrize("c", [c for c in L.FOCAL_CASES if c["N"] <= 1025], ids=lambda c: c["id"])
def test_focal_ref_agrees_with_the_oracle(c):
    x, t = L.focal_inputs(c)
    loss, g = L.focal_ref(x, t, c["gamma"])
    want, want_g = SO.focal_loss(x, t, c["gamma"])
    # the oracle forms logsumexp as m + log(sum): at logits of 3e4 that keeps 4e-12 of absolute precision
    tol = 1e-9 if c["regime"] == "shift" else 1e-12
    assert _rel(loss, want) <= tol and _rel(g, want_g) <= tol


def test_det_loss_restatements_agree(fresh):
    """det_loss_ref (moved here from test_gpu_split.py) against the independently written float32 torch form: same NaN pattern
    (asserted while the table is built), values within the float32 error of the formula"""
    assert fresh[0][("detloss.out", "all")] <= 1e-5


def test_restatements_agree_with_their_float32_forms(fresh):
    for (kind, reg), e in fresh[0].items():
        # peaky softmaxes (amplitude 12 / 30) make the float32 score gradient a difference of nearly equal terms: the reason the kernel
        # computes in double (csrc/proposals.hip)
        assert e <= (0.05 if kind.startswith("scores_bwd") else PIN), (kind, reg, e)


# ------------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("c", L.RPN_CASES, ids=lambda c: c["id"])
def test_rpn_case_keeps_its_distance_from_the_l1_kink(fresh, c):
    """every foreground |delta - target| in float64 is >= 1e-3, or belongs to the exact-zero group and is exactly 0"""
    r = fresh[1]["rpn"][c["id"]]
    ref, i = r["ref"], r["inp"]
    in_zero = np.isin(ref["fg"], i["zero"])
    e = np.abs(ref["err"])
    assert np.all(e[~in_zero] >= 1e-3) and np.all(e[in_zero] == 0.0)
    assert int(in_zero.sum()) == len(i["zero"])
    if c["labels"] in ("mixed", "allfg") and c["A"] >= 255:
        assert len(i["zero"]) == len(L.RPN_ZERO_BOX)
    # the float32 evaluation lands on the same side everywhere: the sign gradient is a bit-exact expectation
    assert np.array_equal(np.sign(r["f32"]["ddeltas"]), np.sign(ref["ddeltas"]))
    lab = i["labels"]
    assert {"mixed": {-1, 0, 1}, "ignore": {-1}, "nofg": {-1, 0}, "allfg": {1}}[c["labels"]] >= set(np.unique(lab).tolist())
    if c["N"] * c["A"] >= 64 and c["labels"] != "ignore":
        part = i["logits"][lab >= 0]
        assert all(np.any(part == v) for v in L.RPN_PLANTED)


def test_rpn_cases_hold_the_launch_edges():
    sizes = {(c["N"], c["A"]) for c in L.RPN_CASES}
    assert sizes >= {(1, 1), (1, 255), (1, 256), (1, 257), (2, 417), (1, 65536), (1, 65537), (3, 21900)}
    assert 65536 % 21900 != 0 and 3 * 21900 > 65536                           # the anchor index wraps inside the second pass
    for mode in ("mixed", "ignore", "nofg", "allfg"):                          # every label kind also in the second pass
        assert any(c["labels"] == mode and c["N"] * c["A"] > 65536 for c in L.RPN_CASES)
    assert {c["w"] for c in L.RPN_CASES} == {"w1", "wreg"}
    # the exact-zero group of a second-pass case reaches beyond the first pass
    i = L.rpn_inputs(dict(N=3, A=21900, labels="mixed", w="wreg"))
    assert i["zero"].min() >= 2 * 21900


def test_focal_cases_hold_every_shape_gamma_and_regime():
    assert {(c["N"], c["C"]) for c in L.FOCAL_CASES if c["gamma"] == 1.5} >= set(L.FOCAL_SHAPES)
    for g in (0.0, 1.0, 2.0):
        assert len({(c["N"], c["C"]) for c in L.FOCAL_CASES if c["gamma"] == g}) >= 4
    assert {c["regime"] for c in L.FOCAL_CASES} == {"sd3", "sd40", "shift", "sep"}
    for C in (1, 2, 63, 64, 65, 1231):
        ld, ld_d = L.focal_layout(C)
        assert ld >= 5 * (C - 1) + 1 and ld != ld_d and ld != C and ld_d != C


def test_detloss_cases_hold_the_launch_edges():
    by = {c["id"]: c for c in L.DETLOSS_CASES}
    assert by["img65"]["N"] == 65 and set(by["img65"]["counts"]) == {0, 1, 63, 64, 65} and by["img65"]["max_rows"] == 65
    assert all(f"A{A}" in by for A in (1, 4095, 4096, 4097))
    assert by["K80"]["counts"] == [64, 65, 128, 129] and by["K1"]["max_rows"] == 129
    assert by["rows100"]["max_rows"] == 100 and 100 in by["rows100"]["counts"] and by["rows100"]["pad"] == 0
    assert by["rows0"]["max_rows"] == 0 and not any(by["rows0"]["counts"])
    assert L.detloss_inputs(by["rows0"])[5].shape == (0, 5 * 20 + 1 + by["rows0"]["pad"])
    c = by["badclass"]
    cls, cnt = L.detloss_inputs(c)[6].numpy(), c["counts"]
    o = sum(cnt[:c["bad_image"]])
    assert (cls[o:o + cnt[c["bad_image"]]] == c["K"] + 1).sum() == 2 and (cls == c["K"] + 1).sum() == 2
    for c in L.DETLOSS_CASES:
        assert all(n <= c["max_rows"] for n in c["counts"])


def test_scores_bwd_cases_span_the_dynamic_lds_range():
    ks = sorted(c["K"] for c in L.SCORES_BWD_CASES)
    assert L.scores_bwd_lds_bytes(63) == 64 * 1024 and 64 in ks and 63 in ks
    assert L.scores_bwd_lds_bytes(159) == 160 * 1024 and max(ks) == 159 and L.scores_bwd_lds_bytes(L.SCORES_BWD_REFUSED[0]) > 160 * 1024
    assert {c["R"] for c in L.SCORES_BWD_CASES} >= {1, 127, 128, 129}
    assert len(set(L.scores_bwd_layout(20))) == 3


@pytest.mark.parametrize("c", L.SELECT_CASES, ids=lambda c: c["id"])
def test_select_case_holds_what_its_kind_says(c):
    scores, classes, boxes, thres = L.select_inputs(c)
    with np.errstate(invalid="ignore"):
        kept = int((scores > np.float32(thres)).sum())
    if c["kind"] == "ties":
        assert int((scores == np.float32(thres)).sum()) > 0
    if c["kind"] == "all":
        assert kept == c["n"]
    if c["kind"] == "none":
        assert kept == 0
    if c["kind"] in ("nonfinite", "neginf"):
        assert np.isnan(scores).any() and np.isposinf(scores).any() and np.isneginf(scores).any()
        assert all(np.isnan(scores[k]) or np.isinf(scores[k]) for k in (0, min(1023, c["n"] - 1), c["n"] - 1))
    if c["kind"] == "neginf":
        assert kept == int(np.isfinite(scores).sum() + np.isposinf(scores).sum())
    assert len(SO.threshold_bbox(scores, classes, boxes, thres, [])[3]) == 0          # an empty label set keeps nothing


# ------------------------------------------------------------------------------------------------ the table
def test_tolerance_table_is_current(fresh):
    """losses_ref.E32 against a fresh computation: the same keys, and every bar max(2e-5, 8 * e32) within a factor 2 of the fresh one
    (below the 2e-5 floor an e32 is rounding noise of this host's float32 kernels and decides nothing)"""
    tab, _ = fresh
    assert set(tab) == set(L.E32), (set(tab) ^ set(L.E32))
    for key, e in tab.items():
        if key[0].startswith(("scores_bwd", "detloss")):                        # kept for the record: these kernels have fixed bars
            continue
        a, b = max(L.BAR_FLOOR, L.BAR_FACTOR * e), L.bar(*key)
        assert a <= 2 * b and b <= 2 * a, (key, e, L.E32[key])


if __name__ == "__main__":
    for key, e in sorted(fresh_table()[0].items()):
        print(f"    {key!r}: {e:.2e},")
