"""CPU: the float64 restatements of tests/heads_ref.py against what the project already trusts (oracle.wsddn_loss, oracle.oicr_losses,
oracle.apply_deltas in float32 + autograd, the inference fixture), the input conditions the GPU edge tests of tests/test_gpu_heads.py
rely on (distance of every image score from the clamp bounds, of every box difference from the kink of the L1 loss), and the
tolerance table heads_ref.E32 (recomputed here; `python tests/test_heads_ref_cpu.py` prints a fresh table)."""
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
from oracle import oicr_oracle as O  # noqa: E402
import heads_ref as H  # noqa: E402

# a wrong restatement is off by O(1); float32 against float64 of these formulas stays far below this at every case used
PIN = 1e-3


def _note(tab, kind, regime, f32, f64):
    e = H.rel_err(f32, f64)
    tab[(kind, regime)] = max(tab.get((kind, regime), 0.0), e)
    return e


def fresh_table():
    """-> (e32 table, per-case records) over every case of the GPU tests"""
    tab, rec = {}, {"wsddn": {}, "refine": {}}
    for c in H.WSDDN_CASES:
        V, R, K = c["V"], c["R"], c["K"]
        cls_col, det_col = H.wsddn_layout(K, c["layout"])[:2]
        lg, gt, gs = H.wsddn_inputs(c)
        ref = H.wsddn_ref(np.nan_to_num(lg).astype(np.float64), V, R, K, cls_col, det_col, gt, gs)
        f32 = H.wsddn_f32(lg, V, R, K, cls_col, det_col, gt, gs)
        reg = H.wsddn_tol_regime(c)
        errs = [_note(tab, "wsddn.scores", reg, f32["scores"], ref["scores"]), _note(tab, "wsddn.loss", reg, f32["loss"], ref["loss"]),
                _note(tab, "wsddn.mean", reg, f32["mean"], ref["mean"]),
                _note(tab, "wsddn.grad", reg, np.concatenate([f32["dcls"], f32["ddet"]], 2), np.concatenate([ref["dcls"], ref["ddet"]], 2))]
        rec["wsddn"][c["id"]] = dict(errs=errs, raw=ref["raw"], clamped=ref["clamped"])
    for c in H.MEAN_PROBS_CASES:
        cls_col, _, stride, _ = H.head_layout(c["K"], c["NR"])
        lg = np.nan_to_num(H.mean_probs_inputs(c))
        a = (c["V"], c["R"], c["K"], c["NR"], cls_col, stride)
        _note(tab, "mean_probs", f"sd{c['sd']:g}", H.mean_probs_f32(lg, *a), H.mean_probs_ref(lg.astype(np.float64), *a))
    for c in H.REFINE_CASES:
        i = H.refine_inputs(c)
        a = (c["V"], c["R"], c["K"], i["cls_col"], i["box_col"], i["boxes"], i["lab_class"], i["lab_weight"], i["lab_index"],
             i["pred_view"], H.REG_WEIGHTS, i["grad_scale"], c["NR"], i["stride"])
        ref = H.refine_ref(np.nan_to_num(i["logits"]).astype(np.float64), *a)
        f32 = H.refine_f32(i["logits"], *a)
        reg = H.refine_tol_regime(c)
        errs = [_note(tab, "refine.loss_cls", reg, f32["loss"][:, 0], ref["loss"][:, 0]),
                _note(tab, "refine.loss_box", reg, f32["loss"][:, 1], ref["loss"][:, 1]),
                _note(tab, "refine.dcls", reg, f32["dcls"], ref["dcls"]), _note(tab, "refine.dbox", reg, f32["dbox"], ref["dbox"])]
        rec["refine"][c["id"]] = dict(errs=errs, min_l1=ref["min_l1"])
    for c in H.PREDICT_CASES:
        lg, boxes, base, stride = H.predict_inputs(c)
        lg = np.nan_to_num(lg)
        a = (c["R"], c["K"], c["RK"], base, stride, boxes, H.REG_WEIGHTS, c["clamp"])
        s32, b32 = H.predict_f32(lg, *a); s64, b64 = H.predict_ref(lg.astype(np.float64), *a)
        _note(tab, "predict.scores", "all", s32, s64); _note(tab, "predict.boxes", "all", b32, b64)
    for n, V, B in H.FINALIZE_CASES:
        lv = H.finalize_inputs(n, V, B)
        o32, t32 = H.loss_finalize_f32(lv); o64, t64 = H.loss_finalize_ref(lv.astype(np.float64))
        _note(tab, "finalize.out", "all", o32, o64); _note(tab, "finalize.total", "all", t32, t64)
    for M, N, nv, _, _, with_g in H.SCALE_COLS_CASES:
        src, gl, gt, c2l, mul = H.scale_cols_inputs(M, N, nv)
        a = (gl if with_g else None, gt, c2l, mul, nv)
        _note(tab, "scale_cols.f32", "all", H.scale_cols_loss_f32(np.nan_to_num(src), *a),
              H.scale_cols_loss_ref(np.nan_to_num(src).astype(np.float64), *a))
    for V, n in H.MEAN_VIEWS_CASES:
        x = H.mean_views_inputs(V, n)
        _note(tab, "mean_views", "all", H.mean_views_f32(x), H.mean_views_ref(x.astype(np.float64)))
    return tab, rec


@pytest.fixture(scope="module")
def fresh():
    return fresh_table()


def test_restatements_agree_with_the_float32_oracle_forms(fresh):
    """every float64 restatement against the float32 form built on oracle.wsddn_loss / oicr_losses / apply_deltas, on every GPU case"""
    tab, _ = fresh
    # the one ill-conditioned corner is the BCE gradient 1 / (1 - y) at the wide logits of regimes b15 / b40, where image scores come
    # within 1e-5 of 1: a float32 y carries an absolute error of about 1e-7 against 1 - y >= 1e-6, up to 10 % of one class's term
    for (kind, reg), e in tab.items():
        assert e <= (0.1 if kind == "wsddn.grad" and reg.startswith("b") else PIN), (kind, reg, e)


@pytest.mark.parametrize("c", H.WSDDN_CASES, ids=[c["id"] for c in H.WSDDN_CASES])
def test_wsddn_case_keeps_its_distance_from_the_clamp(fresh, c):
    r = fresh[1]["wsddn"][c["id"]]
    assert H.clamp_distance_ok(r["raw"]), r["raw"]
    if c["regime"] == "e":                                     # the saturated classes are saturated
        assert r["clamped"].any() and (c["K"] > 2 or r["clamped"].all())
    if c["K"] == 1:
        assert r["clamped"].all() and np.all(r["raw"] > float(H.CLAMP_HI))


@pytest.mark.parametrize("c", H.REFINE_CASES, ids=[c["id"] for c in H.REFINE_CASES])
def test_refine_case_keeps_its_distance_from_the_l1_kink(fresh, c):
    """no |pred - target| below 1e-4 (1 + |target|) except the differences that are exactly zero by construction (labels 'self')"""
    assert fresh[1]["refine"][c["id"]]["min_l1"] >= 1e-4


def test_refine_ref_on_the_inputs_of_the_existing_gpu_tests():
    """refine_ref against oracle.oicr_losses + autograd on the inputs of test_gpu_kernels.test_refine_loss_and_grad"""
    for R, K in ((500, 20), (300, 80)):
        V = 4
        LD = (4 + (K + 1) + 4 * K + 7 + 7) // 8 * 8
        cls_col, box_col = 4, 4 + K + 1
        lg = (torch.randn((V * R, LD), generator=torch.Generator().manual_seed(50)) * 2.0).numpy()
        views, _ = O.make_views(256, 320, R, tag="rl")
        gen = torch.Generator().manual_seed(51)
        lab_class = torch.randint(-1, K + 1, (R,), generator=gen).numpy()
        lab_index = torch.randint(0, R, (R,), generator=gen).numpy()
        lab_weight = torch.rand(R, generator=gen).numpy()
        boxes = np.stack([v["boxes"] for v in views])
        a = (V, R, K, cls_col, box_col, boxes, lab_class, lab_weight, lab_index, [0, 1, 2, 2], H.REG_WEIGHTS, [0.9, 1.3])
        ref = H.refine_ref(lg.astype(np.float64), *a); f32 = H.refine_f32(lg, *a)
        assert H.rel_err(f32["loss"], ref["loss"]) <= 1e-5
        assert H.rel_err(f32["dcls"], ref["dcls"]) <= 1e-5 and H.rel_err(f32["dbox"], ref["dbox"]) <= 1e-5


def test_predict_ref_against_the_inference_fixture_and_the_oracle(golden_dir):
    """the decode of oracle.oicr_plus_inference restated on its own head logits: all_scores against tests/golden/infer_s0.npz (the
    fixture stores no all_boxes), scores and boxes against the oracle's intermediates"""
    e = np.load(os.path.join(golden_dir, "e2e_s0.npz")); g = np.load(os.path.join(golden_dir, "infer_s0.npz"))
    K = 20
    P = O.make_params(K, tuple(int(x) for x in e["dan"]), tag="ps0", head_scale=float(e["head_scale"]))
    views, _ = O.make_views(int(e["H"]), int(e["W"]), int(e["R"]), n_gt=int(e["n_gt"]), K=K, tag="vs0")
    img, boxes, obj = views[0]["image"], views[0]["boxes"], views[0]["obj"]
    o = O.oicr_plus_inference(P, img, boxes, obj, K=K)
    Pt = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in P.items()}
    with torch.no_grad():
        f = O.vgg16_forward(O.preprocess(torch.from_numpy(img))[None], Pt)
        pooled = O._RoIPoolFn.apply(f, O.boxes_to_rois(torch.from_numpy(boxes)), 1.0 / 8, 7, 7)
        hv = O.box_head_forward(pooled * (torch.from_numpy(obj) + 1).view(-1, 1, 1, 1), Pt, None)
        blocks = []
        for k in range(4):
            pre = f"roi_heads.box_refinery_{k}"
            blocks += [F.linear(hv, Pt[pre + ".cls_score.weight"], Pt[pre + ".cls_score.bias"]),
                       F.linear(hv, Pt[pre + ".bbox_pred.weight"], Pt[pre + ".bbox_pred.bias"])]
        lg = torch.cat(blocks, 1).numpy()
    R = boxes.shape[0]
    sc, bx = H.predict_ref(lg.astype(np.float64), R, K, 4, 0, 5 * K + 1, boxes, H.REG_WEIGHTS, H.SCALE_CLAMP)
    Hh, Ww = img.shape[1:]
    bx = bx.reshape(R, K, 4).copy()
    bx[..., 0::2] = bx[..., 0::2].clip(0, Ww); bx[..., 1::2] = bx[..., 1::2].clip(0, Hh)
    assert H.rel_err(o["all_scores"], sc) <= 1e-5 and H.rel_err(o["all_boxes"], bx.reshape(R, 4 * K)) <= 1e-5
    assert H.rel_err(g["all_scores"][0], sc) <= 1e-4          # the fixture's numbers come from another host's float32 sums


def test_mining_sweep_reaches_every_launch_form():
    forms = {H.mine_form(c["R"], H.mine_top_k(c["R"]), c["G"]) for c in H.MINE_CASES}
    assert forms == {"staged", "lds", "ws"}
    assert all(c["G"] <= min(c["K"], 18) for c in H.MINE_CASES)


def test_mean_probs_cases_span_the_dynamic_lds_range():
    sizes = [H.mean_probs_lds_bytes(c["V"], c["K"]) for c in H.MEAN_PROBS_CASES]
    assert any(64 * 1024 < s <= 150 * 1024 for s in sizes) and max(sizes) <= 150 * 1024
    assert H.mean_probs_lds_bytes(*H.MEAN_PROBS_TOO_BIG) > 150 * 1024


def test_tolerance_table_is_current(fresh):
    """heads_ref.E32 against a fresh computation: the same keys, and every bar max(2e-5, 8 * e32) within a factor 2 of the fresh one
    (below the 2e-5 floor an e32 is rounding noise of this host's float32 kernels and decides nothing)"""
    tab, _ = fresh
    assert set(tab) == set(H.E32), (set(tab) ^ set(H.E32))
    for key, e in tab.items():
        a, b = max(H.BAR_FLOOR, H.BAR_FACTOR * e), H.bar(*key)
        assert a <= 2 * b and b <= 2 * a, (key, e, H.E32[key])


if __name__ == "__main__":
    for key, e in sorted(fresh_table()[0].items()):
        print(f"    {key!r}: {e:.2e},")
