"""GPU: OICRPlusHeads' other mining rules — top-1 seeds (WSL.REFINE_MIST False) and box update (OICRPLUS.BBOX_UPDATE True).

sw_oicr_update_boxes against float64 inside the decode bar of oicr_modes_ref.py; sw_oicr_mine_label with class-specific candidate
boxes, both seed rules, lab_box / pgt_box, bit for bit against the reference-written fixtures and the float32 restatement;
sw_oicr_refine_loss with view-0 target boxes against float64; and the three end-to-end fixtures through the whole model."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import heads_ref as H  # noqa: E402
import oicr_modes_ref as M  # noqa: E402
from helpers import build_model, load_params, to_batched_inputs  # noqa: E402
from oracle import oicr_oracle as O  # noqa: E402

_SENT = 0x7FA51234 - (1 << 32) if False else 0x7FA51234


@pytest.fixture(scope="module")
def ops():
    import sos_wsod_amd.ops as ops
    return ops


def _sent(*shape, dtype=torch.float32):
    t = torch.full(shape, _SENT, device="cuda", dtype=torch.int32)
    return t.view(torch.float32) if dtype == torch.float32 else t


def _untouched(t):
    return (t.view(torch.int32) == _SENT).all().item()


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


# ------------------------------------------------------------------------------------------------ sw_oicr_update_boxes
@pytest.mark.parametrize("V,R,K,G", [(4, 65, 5, 5), (4, 1, 20, 1), (1, 65, 20, 3), (1, 1, 1, 1), (4, 300, 20, 2)])
def test_update_boxes_against_float64(ops, V, R, K, G):
    lg, box_col, boxes, gt, signs, d = M.decode_inputs(V, R, K, G, 100 * V + R + K + G)
    n_heads = 1
    out = _sent(n_heads * R * G * 4 + 8)
    ops.oicr_update_boxes(_cu(lg), V, R, K, n_heads, box_col, 0, _cu(boxes), _cu(gt.astype(np.int32)), _cu(signs), M.WEIGHTS,
                          M.SCALE_CLAMP, out[4:4 + R * G * 4])
    torch.cuda.synchronize()
    assert _untouched(out[:4]) and _untouched(out[4 + R * G * 4:])
    got = out[4:4 + R * G * 4].view(R, G, 4).cpu().numpy().astype(np.float64)
    dg = d[:, :, gt]
    ref, bar = M.decode(dg, boxes, signs), M.decode_bar(dg, boxes)
    assert np.isfinite(got).all()
    print(f"V{V} R{R} K{K} G{G}: max err / bar {float((np.abs(got - ref) / bar).max()):.3f}")
    assert (np.abs(got - ref) <= bar).all()
    clamped = np.minimum(M.mean_deltas(dg, signs)[..., 2] / 5.0, M.SCALE_CLAMP) == M.SCALE_CLAMP
    if R >= 65:
        assert clamped.any() and not clamped.all()                         # dw on both sides of the clamp


def test_update_boxes_two_heads_and_column_stride(ops):
    V, R, K, G = 4, 37, 20, 2
    lg0, box_col, boxes, gt, signs, d0 = M.decode_inputs(V, R, K, G, 7)
    lg1, _, _, _, _, d1 = M.decode_inputs(V, R, K, G, 8)
    lg = np.concatenate([lg0, lg1], 1)
    out = _sent(2, R, G, 4)
    ops.oicr_update_boxes(_cu(lg), V, R, K, 2, box_col, lg0.shape[1], _cu(boxes), _cu(gt.astype(np.int32)), _cu(signs), M.WEIGHTS,
                          M.SCALE_CLAMP, out)
    torch.cuda.synchronize()
    for k, d in enumerate((d0, d1)):
        dg = d[:, :, gt]
        assert (np.abs(out[k].cpu().numpy().astype(np.float64) - M.decode(dg, boxes, signs)) <= M.decode_bar(dg, boxes)).all()


# ------------------------------------------------------------------------------------------------ sw_oicr_mine_label
def _mine(ops, scores, boxes, gt, K, cand=None, cand_from=0, seed_rule=0, ext=True, top_p=0.10, iou_bg=0.5):
    """one launch over scores [NR][R][ncol]; -> dict of host arrays per round, after checking sentinels and a second, bit-equal launch"""
    scores = np.asarray(scores, np.float32)
    NR, R, _ = scores.shape
    G = len(gt)
    top_k = max(int(R * top_p), 1) if seed_rule == 0 else 1
    n = top_k * G
    runs = []
    for _ in range(2):
        b = dict(lab_c=_sent(NR, R, dtype=torch.int32), lab_w=_sent(NR, R), lab_i=_sent(NR, R, dtype=torch.int32),
                 cnt=_sent(NR, dtype=torch.int32), pi=_sent(NR, n, dtype=torch.int32), pc=_sent(NR, n, dtype=torch.int32), ps=_sent(NR, n),
                 lab_b=_sent(NR * R * 4 + 8), pb=_sent(NR, n, 4))
        ws = torch.empty(ops.mine_workspace_bytes(R, top_k, G, NR), dtype=torch.uint8, device="cuda")
        kw = {}
        if ext:
            kw = dict(cand_boxes=None if cand is None else _cu(np.asarray(cand, np.float32)), cand_from=cand_from, seed_rule=seed_rule,
                      lab_box=b["lab_b"][4:4 + NR * R * 4], pgt_box=b["pb"])
        ops.oicr_mine_label(_cu(scores), _cu(np.asarray(gt, np.int32)), _cu(boxes), K, top_k, 0.05, 0.01, iou_bg, 0.6, b["lab_c"],
                            b["lab_w"], b["lab_i"], b["cnt"], b["pi"], b["pc"], b["ps"], ws, **kw)
        torch.cuda.synchronize()
        runs.append({k: v.cpu() for k, v in b.items()})
    for k in runs[0]:
        assert torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)), f"two launches differ in {k}"
    b = runs[0]
    if ext:
        assert _untouched(b["lab_b"][:4]) and _untouched(b["lab_b"][4 + NR * R * 4:])
    else:
        assert _untouched(b["lab_b"]) and _untouched(b["pb"])
    out = []
    for k in range(NR):
        m = int(b["cnt"][k])
        assert 1 <= m <= n
        assert _untouched(b["pi"][k, m:]) and _untouched(b["pc"][k, m:]) and _untouched(b["ps"][k, m:])
        if ext:
            assert _untouched(b["pb"][k, m:])
        out.append(dict(pgt_index=b["pi"][k, :m].numpy(), pgt_class=b["pc"][k, :m].numpy(), pgt_score=b["ps"][k, :m].numpy(),
                        pgt_box=b["pb"][k, :m].numpy(), lab_class=b["lab_c"][k].numpy(), lab_index=b["lab_i"][k].numpy(),
                        lab_weight=b["lab_w"][k].numpy(), lab_box=b["lab_b"][4:4 + NR * R * 4].view(NR, R, 4)[k].numpy()))
    return out


def _same(got, p, l, what, boxes_too=True):
    assert np.array_equal(got["pgt_index"], p["index"]) and np.array_equal(got["pgt_class"], p["classes"]), what
    assert np.array_equal(_bits(got["pgt_score"]), _bits(p["scores"])), what
    assert np.array_equal(got["lab_class"], l["gt_classes"]) and np.array_equal(got["lab_index"], l["gt_index"]), what
    assert np.array_equal(_bits(got["lab_weight"]), _bits(l["gt_weights"])), what
    if boxes_too:
        assert np.array_equal(_bits(got["pgt_box"]), _bits(p["boxes"])), what
        assert np.array_equal(_bits(got["lab_box"]), _bits(l["gt_boxes"])), what


@pytest.mark.parametrize("name", list(M.CASES))
def test_mining_reproduces_the_reference_fixtures_bit_for_bit(ops, name):
    """fed the fixture's scores and its class-specific boxes (so nothing hangs on exp): all four rounds in one launch, STAGED form"""
    g = M.load_case(name)
    _, refine_mist, bbox_update = M.CASES[name]
    _, views, gt, _ = M.case_inputs(g)
    boxes, K, R = views[0]["boxes"], int(g["K"]), int(g["R"])
    gt_int = g["gt_int"]
    scores = np.zeros((4, R, K + 1), np.float32)
    for k in range(4):
        s = g[f"r{k}/scores"]
        scores[k, :, :s.shape[1]] = s
    cand = np.stack([g[f"r{k}/cand_boxes"] for k in range(1, 4)]) if bbox_update else None
    got = _mine(ops, scores, boxes, gt_int, K, cand, 1 if bbox_update else 0, 0 if refine_mist else 1)
    for k in range(4):
        p = dict(index=g[f"r{k}/pgt_index"], classes=g[f"r{k}/pgt_classes"], scores=g[f"r{k}/pgt_scores"], boxes=g[f"r{k}/pgt_boxes"])
        l = dict(gt_classes=g[f"r{k}/gt_classes"], gt_index=g[f"r{k}/gt_index"], gt_weights=g[f"r{k}/gt_weights"], gt_boxes=g[f"r{k}/gt_boxes"])
        _same(got[k], p, l, f"{name} round {k}")


@pytest.mark.parametrize("name", list(M.EDGE_CASES))
def test_mining_edge_cases_against_the_restatement(ops, name):
    c = M.edge_case(name)
    p, l = M.mine_and_label(c["scores"], c["boxes"], c["gt"], c["K"], c["cand"], c["seed_rule"])
    cand = None if c["cand"] is None else c["cand"][None]
    got = _mine(ops, c["scores"][None], c["boxes"], c["gt"], c["K"], cand, 0, c["seed_rule"])[0]
    _same(got, p, l, name)


def test_mining_pairwise_iou_edge_pairs(ops):
    """pairwise_iou at its edges through the labels, with iou_bg = 0 so that an IoU of exactly 0 (ignore, -1) and a NaN or negative one
    (background) part ways; expected from the oracle's pairwise_iou and matcher at thresholds (0, 0.6).  One seed (row 0, class 3):
    a zero-area seed against itself and its twin must give 0, not 0 / 0; a box sharing only an edge gives exactly 0; a proposal with
    a NaN coordinate counts as 0 in the extended kernel (the plain one leaves the NaN, which never wins)"""
    K, gt = 20, np.array([3], np.int64)
    flat, seed = [30, 30, 30, 40], [10, 10, 20, 20]
    runs = {"zero_area": (False, [flat, flat, [30, 30, 40, 40], [100, 100, 110, 110]]),
            "edge": (False, [seed, [20, 10, 30, 20], [12, 10, 22, 20], [100, 100, 110, 110]]),
            "nan": (True, [seed, [np.nan, 10, 20, 20], [10, 10, 20, np.nan], [20, 10, 30, 20]])}
    for name, (ext, bx) in runs.items():
        boxes = np.array(bx, np.float32)
        scores = np.full((1, len(boxes), K + 1), 0.01, np.float32)
        scores[0, 0, 3] = 0.9
        got = _mine(ops, scores, boxes, gt, K, ext=ext, iou_bg=0.0)[0]
        assert got["pgt_index"].tolist() == [0], name
        m, lab = M.O.matcher(M.O.pairwise_iou(boxes[:1], boxes), thresholds=(0.0, 0.6))
        want = np.where(lab == 1, 3, np.where(lab == 0, K, -1))
        assert np.array_equal(got["lab_class"], want), f"{name}: labels {got['lab_class'].tolist()}, the oracle's {want.tolist()}"
        assert want.tolist() == {"zero_area": [-1, -1, -1, -1], "edge": [3, -1, 3, -1], "nan": [3, -1, -1, -1]}[name]


def test_mining_ranks_signed_zeros_and_nan_scores_by_their_bits(ops):
    """make_key orders a score column by the bits of the monotone map, not by value: +0.0 ranks above -0.0 (a value order would tie and
    take the lower row), every negative score below both, and a +NaN above everything.  Only the seed (rank 0) passes the score
    threshold here, so the list is the top of the column"""
    K, R, gt = 20, 24, np.array([3], np.int64)
    gx, gy = np.meshgrid(np.arange(6), np.arange(4))
    boxes = np.stack([gx.ravel() * 40.0, gy.ravel() * 40.0, gx.ravel() * 40.0 + 30.0, gy.ravel() * 40.0 + 30.0], 1).astype(np.float32)
    scores = np.zeros((1, R, K + 1), np.float32)
    scores[0, :, 3] = -np.arange(1, R + 1, dtype=np.float32)               # every other row negative, row 23 the most
    scores[0, 2, 3], scores[0, 5, 3] = -0.0, 0.0
    got = _mine(ops, scores, boxes, gt, K, ext=False)[0]
    assert got["pgt_index"].tolist() == [5] and _bits(got["pgt_score"]).tolist() == _bits([0.0]).tolist()
    scores[0, 5, 3] = -0.5                                                  # without the +0.0 the -0.0 leads, bit for bit
    got = _mine(ops, scores, boxes, gt, K, ext=False)[0]
    assert got["pgt_index"].tolist() == [2] and _bits(got["pgt_score"]).tolist() == _bits([-0.0]).tolist()
    scores[0, 7, 3] = np.nan
    got = _mine(ops, scores, boxes, gt, K, ext=False)[0]
    assert got["pgt_index"].tolist() == [7] and np.isnan(got["pgt_score"]).all()


def test_update_boxes_with_nan_size_deltas_gives_the_clamped_box(ops):
    """sw_oicr_update_boxes averages the views' deltas and clamps dw, dh with fminf, which drops a NaN: the box is the one deltas above
    scale_clamp decode to, finite, where the reference's torch.clamp(max=) would keep the NaN"""
    V, R, K, G = 2, 2, 1, 1
    lg = np.zeros((V * R, 4), np.float32)
    lg[0, 2:] = np.nan                                                     # row 0, view 0: the mean of (NaN, 0) is NaN
    lg[1, 2:] = 1e3; lg[3, 2:] = 1e3                                       # row 1: far above scale_clamp * weight in both views
    boxes = np.array([[10, 10, 30, 50]] * 2, np.float32)
    out = _sent(R, G, 4)
    ops.oicr_update_boxes(_cu(lg), V, R, K, 1, 0, 0, _cu(boxes), _cu(np.zeros(G, np.int32)), _cu(np.ones(V, np.int32)), M.WEIGHTS,
                          M.SCALE_CLAMP, out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), out.tolist()
    assert torch.equal(out[0], out[1]), out.tolist()
    assert float(out[0, 0, 2] - out[0, 0, 0]) > 1000.0 and float(out[0, 0, 3] - out[0, 0, 1]) > 2000.0


def test_mining_workspace_form_with_candidate_boxes(ops):
    """beyond the LDS limit (R = 10000, G = 17: the sort keys live in the workspace) the lists and the boxes are looked up in global memory"""
    R, K, G = 10000, 80, 17
    rng = np.random.default_rng(17)
    assert H.mine_form(R, H.mine_top_k(R), G) == "ws"
    boxes = H.random_boxes(rng, R, size=600.0)
    scores = (rng.random((R, K + 1)) ** 8).astype(np.float32)
    gt = np.sort(rng.choice(K, G, replace=False)).astype(np.int64)
    cand = (boxes[:, None, :] + rng.uniform(-6, 6, (R, G, 4))).astype(np.float32)
    p, l = M.mine_and_label(scores, boxes, gt, K, cand, 0)
    got = _mine(ops, scores[None], boxes, gt, K, cand[None], 0, 0)[0]
    _same(got, p, l, "workspace form")
    assert len(p["index"]) > 3 and not np.array_equal(p["boxes"], boxes[p["index"]])


def test_mining_without_the_new_arguments_equals_the_extended_kernel_on_mining_a(ops, golden_dir):
    """NULL / 0 new arguments reach the kernel as it always was; the extended instantiation given no candidates and seed rule 0 must
    give the same lists and labels, and its lab_box is boxes[lab_index]"""
    g = np.load(os.path.join(golden_dir, "mining_a.npz"))
    R, K, gt = int(g["R"]), int(g["K"]), g["gt"]
    views, _ = O.make_views(256, 320, R, n_gt=len(gt), K=K, tag=str(g["boxes_tag"]))
    boxes = views[0]["boxes"]
    sc = g["refine/scores"]
    old = _mine(ops, sc[None], boxes, gt, K, ext=False)[0]
    new = _mine(ops, sc[None], boxes, gt, K, ext=True)[0]
    p = dict(index=g["refine/pgt_index"], classes=g["refine/pgt_classes"], scores=g["refine/pgt_scores"], boxes=boxes[g["refine/pgt_index"]])
    l = dict(gt_classes=g["refine/gt_classes"], gt_index=g["refine/gt_index"], gt_weights=g["refine/gt_weights"], gt_boxes=g["refine/gt_boxes"])
    _same(old, p, l, "default kernel", boxes_too=False)
    _same(new, p, l, "extended kernel, default rule")


def test_mining_refuses_seed_rule_1_with_top_k_above_1(ops):
    R, K = 40, 20
    z = torch.zeros(R, K + 1, device="cuda")
    o = _sent(R, dtype=torch.int32)
    with pytest.raises(Exception, match="sw_oicr_mine_label"):
        ops.oicr_mine_label(z, _cu(np.array([1], np.int32)), torch.zeros(R, 4, device="cuda"), K, 4, 0.05, 0.01, 0.5, 0.6, o, _sent(R), o,
                            o, o, o, _sent(R), torch.empty(4096, dtype=torch.uint8, device="cuda"), seed_rule=1)
    torch.cuda.synchronize()
    assert _untouched(o)


# ------------------------------------------------------------------------------------------------ sw_oicr_refine_loss
def test_refine_loss_with_view0_target_boxes_against_float64(ops):
    """view 0 regresses towards tgt_box0[r]; float64 reference = heads_ref.refine_ref on a 2R-row problem whose extra rows are ignored
    and hold the target boxes (view 0: tgt_box0, other views: their proposal[lab_index]), so its losses and gradients are 1/2 of ours"""
    c = H._rc("share2", 65, 20, 1, "fg", 2.0)
    V, R, K = c["V"], c["R"], c["K"]
    i = H.refine_inputs(c)
    cls_col, box_col, stride, ld = i["cls_col"], i["box_col"], i["stride"], i["ld"]
    rng = np.random.default_rng(5)
    tgt = H.random_boxes(rng, R)
    lg2 = np.zeros((V, 2 * R, ld), np.float64); lg2[:, :R] = np.nan_to_num(i["logits"]).astype(np.float64).reshape(V, R, ld)
    b2 = np.zeros((V, 2 * R, 4), np.float64); b2[:, :R] = i["boxes"]
    for v in range(V):
        b2[v, R:] = tgt if v == 0 else i["boxes"][v][i["lab_index"][0]]
    lc2 = np.concatenate([i["lab_class"][0], np.full(R, -1, np.int32)])[None]
    lw2 = np.concatenate([i["lab_weight"][0], np.zeros(R, np.float32)])[None]
    li2 = np.concatenate([R + np.arange(R), np.arange(R)]).astype(np.int32)[None]
    ref = H.refine_ref(lg2.reshape(V * 2 * R, ld), V, 2 * R, K, cls_col, box_col, b2, lc2, lw2, li2, i["pred_view"], H.REG_WEIGHTS,
                       i["grad_scale"], 1, stride)
    base = H.refine_ref(np.nan_to_num(i["logits"]).astype(np.float64), V, R, K, cls_col, box_col, i["boxes"], i["lab_class"],
                        i["lab_weight"], i["lab_index"], i["pred_view"], H.REG_WEIGHTS, i["grad_scale"], 1, stride)
    lv, dl = _sent(1, 2, V), _sent(V * R, ld)
    ops.oicr_refine_loss(_cu(i["logits"]), V, R, K, cls_col, box_col, _cu(i["boxes"]), _cu(i["lab_class"]), _cu(i["lab_weight"]),
                         _cu(i["lab_index"]), _cu(i["pred_view"]), H.REG_WEIGHTS, lv, dl, _cu(i["grad_scale"]), n_rounds=1,
                         col_stride=stride, tgt_box0=_cu(tgt[None]))
    torch.cuda.synchronize()
    reg = H.refine_tol_regime(c)
    g = np.nan_to_num(dl.view(V, R, ld).cpu().numpy()).astype(np.float64)      # the sentinel outside the head's columns is a NaN
    for kind, got, want in (("refine.loss_cls", lv[0, 0].cpu().numpy(), 2 * ref["loss"][0, 0]),
                            ("refine.loss_box", lv[0, 1].cpu().numpy(), 2 * ref["loss"][0, 1]),
                            ("refine.dcls", g[:, :, cls_col:cls_col + K + 1], 2 * ref["dcls"][0][:, :R]),
                            ("refine.dbox", g[:, :, box_col:box_col + 4 * K], 2 * ref["dbox"][0][:, :R])):
        e, b = H.rel_err(got, want), H.bar(kind, reg)
        print(f"{kind}: err {e:.3g}, bar {b:.3g}")
        assert e <= b, kind
    # the case is one where the view-0 targets matter: view 0's box loss and the sign pattern of the box gradient both change
    assert abs(2 * ref["loss"][0, 1, 0] - base["loss"][0, 1, 0]) > 1e-2 * base["loss"][0, 1, 0]
    assert np.array_equal(2 * ref["loss"][0, 1, 1:], base["loss"][0, 1, 1:])
    assert (np.sign(ref["dbox"][0][0, :R]) != np.sign(base["dbox"][0][0])).any()


# ------------------------------------------------------------------------------------------------ end to end
def _model(g, dtype):
    P, views, gt, masks = M.case_inputs(g)
    model = build_model(int(g["K"]), tuple(int(x) for x in g["dan"]), dtype)
    load_params(model, P)
    model.train()
    model.roi_heads.refine_mist, model.roi_heads.bbox_update = bool(g["refine_mist"]), bool(g["bbox_update"])
    model.roi_heads.debug_drop_masks = [[torch.from_numpy(m) for m in v] for v in masks]
    return model, views, gt


@pytest.mark.parametrize("name", list(M.CASES))
def test_fp32_iteration_matches_the_reference_fixture(name):
    """losses at 1e-4 relative, integer outputs exact, gradient samples at test_gpu_e2e.py's bars for e2e_s0"""
    from sos_wsod_amd.events import EventStorage
    g = M.load_case(name)
    model, views, gt = _model(g, torch.float32)
    with EventStorage(0):
        losses = model(to_batched_inputs(views, gt))
        sum(losses.values()).backward()
    torch.cuda.synchronize()
    for k, v in losses.items():
        ref = float(g["loss/" + k])
        print(name, k, v.item(), ref)
        assert abs(v.item() - ref) <= 1e-4 * abs(ref), (k, v.item(), ref)
    aux = model.roi_heads.last_aux
    boxes = views[0]["boxes"]
    for k in range(4):
        r = aux["rounds"][k]
        n = int(r["pgt_count"].item())
        assert np.array_equal(r["pgt_index"][:n].cpu().numpy(), g[f"r{k}/pgt_index"])
        assert np.array_equal(r["pgt_class"][:n].cpu().numpy(), g[f"r{k}/pgt_classes"])
        assert np.array_equal(r["lab_class"].cpu().numpy(), g[f"r{k}/gt_classes"])
        assert np.array_equal(r["lab_index"].cpu().numpy(), g[f"r{k}/gt_index"])
        np.testing.assert_allclose(r["lab_weight"].cpu().numpy(), g[f"r{k}/gt_weights"], rtol=5e-3)
        if f"r{k}/cand_boxes" in g.files:                  # the GPU's own decode of its own deltas: within the bar of the reference's
            bar = M.decode_bar(g[f"r{k}/deltas"], boxes)
            # (+ the deltas' own difference: a 256-term float32 dot product on either side, 1e-4 relative as for fc7 in test_gpu_e2e.py)
            slack = 1e-4 * (np.abs(g[f"r{k}/cand_boxes"]).max() + 1.0)
            assert (np.abs(r["cand_boxes"].cpu().numpy().astype(np.float64) - g[f"r{k}/cand_boxes"]) <= bar + slack).all()
            np.testing.assert_allclose(r["pgt_box"][:n].cpu().numpy(), g[f"r{k}/pgt_boxes"], rtol=0, atol=float(bar.max() + slack))
            np.testing.assert_allclose(r["lab_box"].cpu().numpy(), g[f"r{k}/gt_boxes"], rtol=0, atol=float(bar.max() + slack))
        else:
            assert np.array_equal(_bits(r["pgt_box"][:n].cpu().numpy()), _bits(g[f"r{k}/pgt_boxes"]))
            assert np.array_equal(_bits(r["lab_box"].cpu().numpy()), _bits(g[f"r{k}/gt_boxes"]))
    sd = dict(model.named_parameters())
    for key in g.files:
        if key.startswith("grad/"):
            ref, got = g[key], sd[key[5:]].grad.cpu().numpy()
        elif key.startswith("grads/"):
            ref, got = g[key], sd[key[6:]].grad.cpu().numpy().ravel()[::997]
        else:
            continue
        tol = 2e-2 if "backbone" in key else 2e-4           # the bars of test_gpu_e2e.py for e2e_s0
        assert np.abs(got - ref).max() <= tol * np.abs(ref).max() + 1e-7, key


@pytest.mark.parametrize("name", list(M.CASES))
def test_bf16_step_runs_to_finite_losses(name):
    from sos_wsod_amd.events import EventStorage
    g = M.load_case(name)
    model, views, gt = _model(g, torch.bfloat16)
    with EventStorage(0):
        losses = model(to_batched_inputs(views, gt))
        sum(losses.values()).backward()
    torch.cuda.synchronize()
    assert len(losses) == 9 and torch.isfinite(losses.vector).all()
    assert torch.isfinite(model.roi_heads.box_head.fc1.weight.grad).all()


def test_step_graph_replay_equals_eager_with_both_switches():
    """the decode launch, the candidate boxes and lab_box live in buffers allocated like the others: the captured step replays"""
    from sos_wsod_amd.solver import HipSGD
    from sos_wsod_amd.trainer import Trainer
    K, dan, R, H_, W = 20, (256, 256), 80, 96, 128
    P = O.make_params(K, dan, tag="pgraph", head_scale=3.0)
    for k in range(4):
        P[f"roi_heads.box_refinery_{k}.bbox_pred.weight"] = P[f"roi_heads.box_refinery_{k}.bbox_pred.weight"] * np.float32(100.0)

    def batches():
        out = []
        for i in range(5):
            views, _ = O.make_views(H_, W, R, n_gt=2, K=K, tag=f"vgraph{i}")
            out.append(to_batched_inputs(views, np.array([(3 + i) % K, (11 + 2 * i) % K]), device="cuda"))
        return out

    def run(use_graph):
        model = build_model(K, dan, torch.bfloat16)
        load_params(model, P)
        model.train()
        model.roi_heads.seed = 77
        model.roi_heads.refine_mist, model.roi_heads.bbox_update = False, True
        groups = [{"params": [p], "lr": 1e-3, "weight_decay": 5e-4} for p in model.parameters() if p.requires_grad]
        tr = Trainer(model, HipSGD(groups, 1e-3, momentum=0.9), use_graph=use_graph, check_finite_every=2, metrics_period=1)
        losses = [tr.run_step(b).vector.detach().clone() for b in batches()]
        tr.finish()
        torch.cuda.synchronize()
        return tr, losses, {n: p.detach().clone() for n, p in model.named_parameters()}
    tr_e, le, we = run(False)
    tr_g, lg, wg = run(True)
    assert tr_g._graphs is not None and tr_g._graphs.captures == 1 and tr_g._graphs.replays == 3
    for i, (a, b) in enumerate(zip(le, lg)):
        assert torch.equal(a, b), (i, a, b)
    assert not [n for n in we if not torch.equal(we[n], wg[n])]
    assert tr_g.raw_model.roi_heads.last_aux["rounds"][1]["cand_boxes"] is not None
