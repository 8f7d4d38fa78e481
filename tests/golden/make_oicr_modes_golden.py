"""Generate tests/golden/oicr_modes_<case>.npz by running the REFERENCE's own OICRPlusHeads (imported through ref_shim.py) with its
other mining rules switched on: `refine_mist` False (top-1 seeds, get_pgt_top_k) and `cfg.OICRPLUS.BBOX_UPDATE` True.

Run in the build container only:   python tests/golden/make_oicr_modes_golden.py

Per case: the recipe of the closed-form inputs (tags, shapes, the bbox_pred scale), and per refinement round the reference's mining
scores, its class-specific candidate boxes (`prev_pred_boxes1`, the image-level classes' columns, float32), the pseudo-GT list
(index, class, score, box), the labels (gt_classes, gt_index, gt_weights, gt_boxes), the nine losses and the gradient samples the
e2e_* fixtures keep.  Data only; nothing of the reference's text.

The decoded boxes differ between hosts and the GPU by a few ulp of exp, so a case is accepted only when every comparison a label
hangs on keeps a margin (oicr_modes_ref.IOU_MARGIN / SCORE_MARGIN) that is larger than the decode bar allows an IoU to move; the
generator walks on to the next seed tag until that holds, until the update changes at least one label (and, where NMS runs, one
NMS decision) against the same inputs without it, and until no loss hangs on pseudo-GT weights out of a softmax tail (conditioning()).
`NAME FIRST COUNT [OUT_DIR]` walks one case over a range of tags, so that ranges can be searched side by side; the committed fixtures
are the first accepted tags: top1 `s0`, upd `s0mupd6` at bbox_pred scale 300, both `s0mboth7` at scale 100.
"""
import os
import sys

os.environ.update({"MKL_CBWR": "COMPATIBLE"})
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
import ref_shim  # noqa: E402
import make_golden as MG  # noqa: E402  (installs the shim; shares load_params / to_batched_inputs / DropoutPatch / the gradient keys)
import oicr_modes_ref as M  # noqa: E402
from oracle import oicr_oracle as O  # noqa: E402

ns = MG.ns
torch.set_num_threads(int(os.environ.get("OICR_MODES_THREADS", torch.get_num_threads())))    # several ranges side by side
K = 20


def run_reference(meta, refine_mist, bbox_update):
    P, views, gt, masks = M.case_inputs(meta)
    model = ref_shim.build_reference_model(ns, K, tuple(int(x) for x in meta["dan"]))
    MG.load_params(model, P)
    model.train()
    heads = model.roi_heads
    heads.refine_mist = refine_mist
    heads.cfg.OICRPLUS.BBOX_UPDATE = bbox_update
    rec = {"pgt": [], "lab": [], "scores": [], "prev": [], "deltas": [[] for _ in range(4)]}
    for k in range(4):                                               # every head's bbox_pred output, views in call order (:373-376)
        heads.box_refinery[k].register_forward_hook(lambda m, i, o, k=k: rec["deltas"][k].append(o[1].detach().numpy().copy()))
    name = "get_pgt_mist" if refine_mist else "get_pgt_top_k"        # get_pgt_mist calls get_pgt_top_k itself: wrap the outer one only
    orig_mine, orig_label = getattr(heads, name), heads.label_and_sample_proposals

    def mine(prev_boxes, prev_scores, *a, **k):
        t = orig_mine(prev_boxes, prev_scores, *a, **k)
        s = prev_scores[0] if isinstance(prev_scores, (list, tuple)) else prev_scores
        rec["pgt"].append(t[0]); rec["scores"].append(s.detach().numpy().copy())
        rec["prev"].append(None if isinstance(prev_boxes[0], ns.boxes.Boxes) else prev_boxes[0].detach().numpy().copy())
        return t

    def label(*a, **k):
        t = orig_label(*a, **k); rec["lab"].append(t[0]); return t
    setattr(heads, name, mine)
    heads.label_and_sample_proposals = label
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self                   # :415-416 move the averaged deltas to the GPU
    try:
        with MG.EventStorage(0), MG.DropoutPatch(masks):
            losses = model(MG.to_batched_inputs(views, gt))
            sum(losses.values()).backward()
    finally:
        torch.Tensor.cuda = orig_cuda
    gt_int = np.unique(np.asarray(gt, np.int64))
    out = {}
    for k in range(4):
        t, l = rec["pgt"][k], rec["lab"][k]
        out[f"r{k}/scores"] = rec["scores"][k].astype(np.float32)
        if rec["prev"][k] is not None:
            assert rec["prev"][k].dtype == np.float32
            out[f"r{k}/cand_boxes"] = rec["prev"][k].reshape(-1, K, 4)[:, gt_int]
            # the float32 deltas of head k-1 the update averaged, image-level classes only: [V][R][G][4]
            out[f"r{k}/deltas"] = np.stack([d.reshape(-1, K, 4)[:, gt_int] for d in rec["deltas"][k - 1][:4]])
        out[f"r{k}/pgt_index"] = t.gt_index.numpy(); out[f"r{k}/pgt_classes"] = t.gt_classes.numpy()
        out[f"r{k}/pgt_scores"] = t.gt_scores.numpy(); out[f"r{k}/pgt_boxes"] = t.gt_boxes.tensor.numpy()
        out[f"r{k}/gt_classes"] = l.gt_classes.numpy(); out[f"r{k}/gt_index"] = l.gt_index.numpy()
        out[f"r{k}/gt_weights"] = l.gt_weights.numpy(); out[f"r{k}/gt_boxes"] = l.gt_boxes.tensor.numpy()
    for k, v in losses.items():
        out["loss/" + k] = np.float64(v.item())
    sd = dict(model.named_parameters())
    for k in MG.GRAD_KEYS_FULL:
        out["grad/" + k] = sd[k].grad.numpy()
    for k in MG.GRAD_KEYS_SAMPLED:
        out["grads/" + k] = sd[k].grad.numpy().ravel()[::MG.SAMPLE_STRIDE]
    return out, views, gt_int


def rel_gap(a, b):
    """relative distance of two scores; two exact zeros (a softmax that underflowed on every host, as in e2e_s1) count as apart:
    their order is the index order everywhere"""
    if float(a) == 0.0 and float(b) == 0.0:
        return 1.0
    return abs(float(a) - float(b)) / max(abs(float(a)), abs(float(b)))


def margins(out, views, gt_int, seed_rule, bar_max):
    """-> list of the margin violations of every comparison a label hangs on (empty: the fixture is robust)"""
    bad = []
    boxes = views[0]["boxes"]
    R, G = boxes.shape[0], len(gt_int)
    for k in range(4):
        sc = out[f"r{k}/scores"]
        cand = out.get(f"r{k}/cand_boxes")
        p, l = M.mine_and_label(sc, boxes, gt_int, K, cand, seed_rule)
        if not (np.array_equal(p["index"], out[f"r{k}/pgt_index"]) and np.array_equal(p["classes"], out[f"r{k}/pgt_classes"])
                and np.array_equal(p["boxes"], out[f"r{k}/pgt_boxes"]) and np.array_equal(l["gt_classes"], out[f"r{k}/gt_classes"])
                and np.array_equal(l["gt_index"], out[f"r{k}/gt_index"]) and np.array_equal(l["gt_boxes"], out[f"r{k}/gt_boxes"])
                and np.array_equal(l["gt_weights"], out[f"r{k}/gt_weights"])):
            bad.append(f"r{k}: the restatement does not reproduce the reference")
        # score orders that select or order a seed
        top_k = max(int(R * 0.10), 1) if seed_rule == 0 else 1
        for g in range(G):
            col = np.sort(sc[:, gt_int[g]].astype(np.float64))[::-1][:top_k + 1]
            for a, b in zip(col[:-1], col[1:]):
                if rel_gap(a, b) < M.SCORE_MARGIN:
                    bad.append(f"r{k}: score order of class {gt_int[g]}: {a} {b}")
            if seed_rule == 0:
                for a in col[1:top_k]:
                    if rel_gap(a, 0.05) < M.SCORE_MARGIN:
                        bad.append(f"r{k}: score {a} at the threshold")
        pre = p["pre_nms"]
        if seed_rule == 0:
            s = np.sort(pre["scores"].astype(np.float64))[::-1]
            for a, b in zip(s[:-1], s[1:]):
                if rel_gap(a, b) < M.SCORE_MARGIN:
                    bad.append(f"r{k}: NMS order {a} {b}")
        if cand is None:
            continue                                    # the boxes are proposal boxes: every IoU is the same bits everywhere
        side = min(float((pre["boxes"][:, 2:] - pre["boxes"][:, :2]).min()), float((boxes[:, 2:] - boxes[:, :2]).min()))
        if not side > 0 or M.iou_sensitivity(side) * bar_max >= M.IOU_MARGIN:
            bad.append(f"r{k}: min side {side}: the decode bar {bar_max} can move an IoU by more than the margin")
            continue
        if seed_rule == 0:
            iou = O.pairwise_iou(pre["boxes"], pre["boxes"]).astype(np.float64)
            near = np.abs(iou - 0.01) < M.IOU_MARGIN
            near &= iou > 0                             # disjoint by more than the bar is checked below through the raw overlap
            if near.any():
                bad.append(f"r{k}: {int(near.sum())} NMS IoUs within the margin of 0.01")
        iou = O.pairwise_iou(p["boxes"], boxes).astype(np.float64)          # (n_pgt, R)
        srt = np.sort(iou, axis=0)[::-1]
        best = srt[0]
        for t in (0.5, 0.6):
            if (np.abs(best - t) < M.IOU_MARGIN).any():
                bad.append(f"r{k}: a matched IoU within the margin of {t}")
        if iou.shape[0] > 1:
            close = (srt[0] - srt[1]) < M.IOU_MARGIN
            # a tie at exactly 0 stays a tie only if every pseudo box is disjoint from the proposal by more than the bar
            gb, pb = p["boxes"].astype(np.float64), boxes.astype(np.float64)
            rw = np.minimum(gb[:, None, 2], pb[None, :, 2]) - np.maximum(gb[:, None, 0], pb[None, :, 0])
            rh = np.minimum(gb[:, None, 3], pb[None, :, 3]) - np.maximum(gb[:, None, 1], pb[None, :, 1])
            disjoint = (np.minimum(rw, rh) < -4 * bar_max).all(axis=0)
            n = int((close & ~((best == 0) & disjoint)).sum())
            if n:
                bad.append(f"r{k}: {n} proposals whose two best IoUs are within the margin")
    return bad


def conditioning(out):
    """-> the largest weight-averaged |ln w| over the rounds.  A classification loss is sum_r w_r CE_r with the pseudo-GT scores as
    weights, and a softmax score carries about |ln w| * 3e-6 of relative float32 noise between two hosts (1.4e-4 was seen at
    w = 2e-22).  The losses are compared at 1e-4, so inputs whose loss hangs on the softmax tail are passed over."""
    worst = 0.0
    for k in range(4):
        w = out[f"r{k}/gt_weights"][out[f"r{k}/gt_classes"] != -1].astype(np.float64)
        w = w[w > 0]
        worst = max(worst, float((w * np.abs(np.log(w))).sum() / w.sum()) if len(w) else np.inf)
    return worst


def generate(name, first=0, count=400, out_dir=HERE):
    """walks the seed tags from `first` on and writes the first one that is accepted"""
    shape, refine_mist, bbox_update = M.CASES[name]
    H, W, R, n_gt, dan, hs = M.SHAPES[shape]
    seed_rule = 0 if refine_mist else 1
    for attempt in range(first, first + count):
        for box_scale in ((100.0, 300.0) if bbox_update else (1.0,)):
            meta = dict(H=H, W=W, R=R, n_gt=n_gt, K=K, dan=np.array(dan), head_scale=hs,
                        tag=shape if attempt == 0 else f"{shape}{name}{attempt}",      # first the e2e_* fixtures' own inputs
                        box_scale=np.float32(box_scale), refine_mist=refine_mist, bbox_update=bbox_update, shape_case=shape)
            out, views, gt_int = run_reference(meta, refine_mist, bbox_update)
            changed_lab = changed_nms = 0
            bar_max = 0.0
            if bbox_update:
                base, _, _ = run_reference(meta, refine_mist, False)
                for k in range(1, 4):
                    changed_lab += int((out[f"r{k}/gt_classes"] != base[f"r{k}/gt_classes"]).sum())
                    changed_nms += int(not (np.array_equal(out[f"r{k}/pgt_index"], base[f"r{k}/pgt_index"])
                                            and np.array_equal(out[f"r{k}/pgt_classes"], base[f"r{k}/pgt_classes"])))
                    bar_max = max(bar_max, float(M.decode_bar(out[f"r{k}/deltas"], views[0]["boxes"]).max()))
            bad = margins(out, views, gt_int, seed_rule, bar_max)
            if conditioning(out) > 5.0:
                bad.append(f"a loss hangs on pseudo-GT weights of mean |ln w| {conditioning(out):.1f}")
            ok = not bad and (not bbox_update or (changed_lab >= 1 and (seed_rule == 1 or changed_nms >= 1)))
            print(f"[oicr_modes {name}] tag {meta['tag']} box_scale {box_scale:g}: labels changed by the update {changed_lab}, "
                  f"rounds whose kept list changed {changed_nms}, bar {bar_max:.2e}, margin violations {len(bad)}"
                  + ("" if not bad else " e.g. " + bad[0]), flush=True)
            if ok:
                out.update(meta)
                out["gt_int"] = gt_int
                out["bar_max"] = np.float64(bar_max)
                np.savez_compressed(os.path.join(out_dir, f"oicr_modes_{name}.npz"), **out)
                print(f"[oicr_modes {name}] losses:", {k[5:]: round(float(v), 6) for k, v in out.items() if k.startswith("loss/")})
                print(f"[oicr_modes {name}] pgt sizes:", [len(out[f'r{k}/pgt_index']) for k in range(4)],
                      "fg:", [int(((out[f'r{k}/gt_classes'] >= 0) & (out[f'r{k}/gt_classes'] < K)).sum()) for k in range(4)])
                return
    raise SystemExit(f"no robust fixture found for {name}")


if __name__ == "__main__":
    torch.manual_seed(0)
    if len(sys.argv) > 2:                                  # one case over a range of seed tags: NAME FIRST COUNT [OUT_DIR]
        generate(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), *(sys.argv[4:5]))
    else:
        for c in (sys.argv[1:] or list(M.CASES)):
            generate(c)
