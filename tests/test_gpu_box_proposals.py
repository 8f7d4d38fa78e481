"""GPU: box-proposal AR (sos_wsod_amd.box_proposals over ops.box_proposal_ar) against the numbers the reference's own
`_evaluate_box_proposals` gave (tests/golden/box_proposal_*.npz) and, round for round, against the NumPy restatement
(box_proposal_ref); the kernel's dispatch edges, memory and refusals; the evaluator end to end; frcnn.ProposalNetwork against
the detector it shares its modules with."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import box_proposal_fixture as F
import box_proposal_ref as R
from test_box_proposals_ref_cpu import same_bits

pytestmark = pytest.mark.gpu

SENTINEL_F, SENTINEL_I, GUARD = -7.5, -77, 96
ALL = [[0.0, 1e10]]


@pytest.fixture(scope="module")
def ops():
    import sos_wsod_amd  # noqa: F401
    import sos_wsod_amd.ops as ops
    return ops


# ------------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", F.CASES)
def test_fixture_case_equals_the_reference_and_the_restatement_round_for_round(golden_dir, name):
    from sos_wsod_amd import box_proposals as BP
    from sos_wsod_amd.evaluation import COCOGroundTruth
    z = F.load(golden_dir, name)
    ds, preds, settings = F.case(name)
    areas = list(dict.fromkeys(a for a, _ in settings))
    limits = list(dict.fromkeys(l for _, l in settings))
    out, stats = BP.box_proposal_metrics(F.records(preds), COCOGroundTruth(ds), areas=areas, limits=limits, return_matches=True)
    for area, limit in settings:
        k, s = F.key(area, limit), stats[area, limit]
        assert s["gt_overlaps"].dtype == torch.float32 and s["recalls"].dtype == torch.float32 and s["ar"].dtype == torch.float32
        assert same_bits(s["gt_overlaps"].numpy(), z[k + "/gt_overlaps"]), k
        assert same_bits(s["recalls"].numpy(), z[k + "/recalls"]) and same_bits(s["ar"].numpy(), z[k + "/ar"]), k
        assert s["num_pos"] == int(z[k + "/num_pos"]) and isinstance(s["num_pos"], int), k
        r = R.evaluate_case(name, area, limit)
        assert [im[0] for im in s["images"]] == [im[0] for im in r["images"]], k
        for got, want in zip(s["images"], r["images"]):
            assert same_bits(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), (k, got[0])
    for (area, limit), key in zip(F.EVALUATOR_SETTINGS, F.EVALUATOR_KEYS):
        if (area, limit) in settings:
            want = float(z[F.key(area, limit) + "/ar100"])
            assert out[key] == want or (np.isnan(out[key]) and np.isnan(want)), key


def test_single_setting_call_returns_the_reference_dict(golden_dir):
    from sos_wsod_amd import box_proposals as BP
    from sos_wsod_amd.evaluation import COCOGroundTruth
    z = F.load(golden_dir, "hand")
    ds, preds, _ = F.case("hand")
    gt = COCOGroundTruth(ds)
    s = BP.evaluate_box_proposals(F.records(preds), gt, area="medium", limit=2)
    assert set(s) == {"ar", "recalls", "thresholds", "gt_overlaps", "num_pos"}
    assert same_bits(s["gt_overlaps"].numpy(), z["medium/2/gt_overlaps"]) and same_bits(s["ar"].numpy(), z["medium/2/ar"])
    assert torch.equal(s["thresholds"], BP.default_thresholds())
    # the arrays of a pickle are scored the same way; custom thresholds reach the kernel
    arrays = [{"image_id": p["image_id"], "boxes": p["boxes"], "objectness_logits": p["logits"]} for p in preds]
    thr = torch.tensor([0.0, 0.3, 0.8], dtype=torch.float32)
    s2 = BP.evaluate_box_proposals(arrays, gt, thresholds=thr, area="all", limit=None)
    r = R.evaluate(ds, preds, thresholds=thr.numpy(), area="all", limit=None)
    assert same_bits(s2["recalls"].numpy(), r["recalls"]) and float(s2["recalls"][0]) == 1.0      # trailing zeros count at 0
    s0 = BP.evaluate_box_proposals(F.records(preds), gt, area="512-inf")
    assert s0["num_pos"] == 0 and torch.isnan(s0["ar"]) and torch.isnan(s0["recalls"]).all() and s0["gt_overlaps"].numel() == 0


# ------------------------------------------------------------------------------------------------------------------- the op
def make_image(rng, P, G, grid=False):
    """(ranked proposals f32 [P, 4], gt boxes f32 [G, 4], areas f32 [G]); Gaussian placement: the coordinates are not
    representable, the division rounds; grid: exact ties and zero-size boxes"""
    if grid:
        xy = rng.integers(0, 20, (G, 2)) * 16.0
        gt = np.concatenate([xy, xy + rng.integers(1, 12, (G, 2)) * 16.0], 1)
        pxy = rng.integers(0, 24, (P, 2)) * 16.0
        prop = np.concatenate([pxy, pxy + rng.integers(0, 12, (P, 2)) * 16.0], 1)
    else:
        xy = rng.uniform(0, 500, (G, 2))
        wh = np.exp(rng.uniform(np.log(6), np.log(300), (G, 2)))
        gt = np.concatenate([xy, xy + wh], 1)
        src = gt[rng.integers(0, G, P)] if G else np.zeros((P, 4))
        near = (rng.random(P) < 0.7)[:, None]
        far_xy = rng.uniform(0, 500, (P, 2))
        far = np.concatenate([far_xy, far_xy + np.exp(rng.uniform(np.log(6), np.log(300), (P, 2)))], 1)
        w, h = (src[:, 2] - src[:, 0])[:, None], (src[:, 3] - src[:, 1])[:, None]
        prop = np.where(near, src + rng.normal(0, 0.12, (P, 4)) * np.concatenate([w, h, w, h], 1), far)
    gt = gt.astype(np.float32)
    area = ((gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]) * rng.uniform(0.3, 1.0, G).astype(np.float32)).astype(np.float32)
    return prop.astype(np.float32).reshape(-1, 4), gt.reshape(-1, 4), area


def expected(images, area_rng, limits, thr):
    """the restatement over a split of make_image tuples -> (item lengths [L * A * n], overlap, match_gt, match_box, cnt [L, A, T])"""
    n = len(images)
    lens, ov, mg, mb = [], [], [], []
    cnt = np.zeros((len(limits), len(area_rng), len(thr)), dtype=np.int64)
    for l, lim in enumerate(limits):
        for a, (lo, hi) in enumerate(area_rng):
            for prop, gt, area in images:
                valid = (area >= np.float32(lo)) & (area <= np.float32(hi))
                if len(prop) == 0 or len(gt) == 0 or not valid.any():
                    lens.append(0)
                    continue
                o, g, p = R.greedy(R.iou_matrix(gt[valid], prop[:lim] if lim else prop))
                lens.append(len(o)); ov.append(o); mg.append(g); mb.append(p)
                cnt[l, a] += [(o >= np.float32(t)).sum() for t in thr]
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)          # noqa: E731
    return np.asarray(lens, dtype=np.int64), cat(ov, np.float32), cat(mg, np.int32), cat(mb, np.int32), cnt


def device_split(images, lens):
    cat = lambda xs, shape: np.concatenate(xs).reshape(shape) if xs else np.zeros(shape, dtype=np.float32)      # noqa: E731
    off = lambda k: np.concatenate([[0], np.cumsum([len(im[k]) for im in images])]).astype(np.int64)             # noqa: E731
    arrays = (off(0), cat([im[0] for im in images], (-1, 4)), off(1), cat([im[1] for im in images], (-1, 4)),
              cat([im[2] for im in images], (-1,)))
    item_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays], torch.from_numpy(item_off).cuda()


def guarded(n):
    """outputs with sentinel-filled guard bands on both sides -> (whole buffers, the views handed to the op)"""
    whole = (torch.full((n + 2 * GUARD,), SENTINEL_F, device="cuda"), torch.full((n + 2 * GUARD,), SENTINEL_I, device="cuda", dtype=torch.int32),
             torch.full((n + 2 * GUARD,), SENTINEL_I, device="cuda", dtype=torch.int32))
    return whole, tuple(w[GUARD:GUARD + n] for w in whole)


def run_and_check(ops, images, area_rng=ALL, limits=(0,), thr=(0.5, 0.75), **kw):
    lens, ov, mg, mb, cnt = expected(images, area_rng, limits, thr)
    dev, item_off = device_split(images, lens)
    whole, views = guarded(len(ov))
    o, g, b, c, status = ops.box_proposal_ar(*dev, area_rng, limits, thr, item_off, overlap=views[0], match_gt=views[1], match_box=views[2], **kw)
    assert int(status.item()) == 0
    assert same_bits(o.cpu().numpy(), ov) and np.array_equal(g.cpu().numpy(), mg) and np.array_equal(b.cpu().numpy(), mb)
    assert np.array_equal(c.cpu().numpy(), cnt) and c.shape == (len(limits), len(area_rng), len(thr))
    for w, s in zip(whole, (SENTINEL_F, SENTINEL_I, SENTINEL_I)):                                # the guard bands stay untouched
        assert bool((w[:GUARD] == s).all()) and bool((w[GUARD + len(ov):] == s).all())
    return dev, item_off, (o, g, b, c)


@pytest.mark.parametrize("P", [1, 63, 64, 65, 1023, 1024, 1025])
def test_proposal_counts_at_the_lane_and_lds_edges(ops, P):
    """P' around the wave width and around SW_BOXAR_LDS_BOXES (beyond it the proposals are read from global memory and the
    state lives in the workspace); Gaussian boxes and grid boxes (ties)"""
    assert ops.BOXAR_LDS_BOXES == 1024
    rng = np.random.default_rng(100 + P)
    run_and_check(ops, [make_image(rng, P, 7), make_image(rng, P, 40, grid=True), make_image(rng, P, 2)])


@pytest.mark.parametrize("G", [1, 63, 64, 65, 128, 129, 200])
def test_box_counts_at_the_lane_and_capacity_edges(ops, G):
    """G' around the wave width and around SW_BOXAR_LDS_GT, with fewer, as many and more proposals than boxes"""
    assert ops.BOXAR_LDS_GT == 128
    rng = np.random.default_rng(200 + G)
    run_and_check(ops, [make_image(rng, 150, G), make_image(rng, G, G, grid=True), make_image(rng, max(G // 2, 1), G)])


def test_one_image_and_the_smallest_call(ops):
    rng = np.random.default_rng(3)
    run_and_check(ops, [make_image(rng, 1, 1)], thr=(0.5,))                                      # n_img = A = L = T = 1, P' = G' = 1
    run_and_check(ops, [make_image(rng, 30, 9, grid=True)], thr=(0.5,))


def test_more_images_than_one_grid_pass_and_images_without_items(ops):
    """the workgroups stride over the images (at most 8 per compute unit in flight); images without proposals, without ground
    truth, or with no box in the range lie between images with items and leave no trace"""
    rng = np.random.default_rng(4)
    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    images = []
    for i in range(n):
        P, G = (0, 2) if i % 7 == 3 else (3, 0) if i % 7 == 5 else (int(rng.integers(1, 6)), int(rng.integers(1, 5)))
        images.append(make_image(rng, P, G, grid=bool(i % 2)))
    images[0] = make_image(rng, 0, 3)
    images[-1] = make_image(rng, 4, 0)
    rng_small = [[0.0, 4000.0], [1e9, 1e10]]                                                    # the second range holds nothing
    run_and_check(ops, images, area_rng=rng_small, limits=(0, 2))


def test_eight_ranges_eight_limits_sixteen_thresholds_at_once(ops):
    rng = np.random.default_rng(5)
    images = [make_image(rng, int(rng.integers(1, 90)), int(rng.integers(1, 30)), grid=bool(i % 3 == 0)) for i in range(12)]
    run_and_check(ops, images, area_rng=[[float(lo), float(hi)] for lo, hi in R.AREA_RANGES], limits=(0, 1, 2, 3, 10, 50, 64, 65),
                  thr=[i / 16 for i in range(16)])


def test_no_limit_next_to_limit_one_and_thresholds_at_or_below_zero(ops):
    """limit 0 means none; with limit 1 only the first round runs and every other box is a trailing zero, which thresholds <= 0
    count"""
    rng = np.random.default_rng(6)
    images = [make_image(rng, 20, 6), make_image(rng, 1, 4), make_image(rng, 9, 1, grid=True)]
    _, _, (o, g, b, c) = run_and_check(ops, images, limits=(0, 1), thr=(-1.0, 0.0, 0.5))
    n_box = sum(len(im[1]) for im in images)
    assert c[:, 0, 0].tolist() == [n_box, n_box] and c[:, 0, 1].tolist() == [n_box, n_box] and int(c[1, 0, 2]) <= len(images)


def test_skipped_regions_stay_untouched_and_two_launches_are_bit_equal(ops):
    """an image without proposals is skipped whatever region item_off gives it (here: one element per box, as if it counted): the
    region keeps the sentinel; so does everything behind item_off[-1]; the same launch twice gives the same bits"""
    rng = np.random.default_rng(7)
    images = [make_image(rng, 0 if i % 5 == 2 else int(rng.integers(1, 300)), int(rng.integers(0, 40)), grid=bool(i % 2)) for i in range(40)]
    images += [make_image(rng, 1100, 30), make_image(rng, 50, 140)]
    limits, thr = (0, 100), (0.5, 0.6, 0.7)
    lens, ov, mg, mb, cnt = expected(images, ALL, limits, thr)
    holes = np.asarray([len(im[1]) if len(im[0]) == 0 else 0 for im in images] * len(limits), dtype=np.int64)
    assert holes.sum() > 0 and (lens[holes > 0] == 0).all()
    dev, item_off = device_split(images, lens + holes)
    keep = np.repeat(holes == 0, lens + holes)                                                  # the elements that items own
    total = int((lens + holes).sum()) + GUARD
    outs = []
    for _ in range(2):
        buf = (torch.full((total,), SENTINEL_F, device="cuda"), torch.full((total,), SENTINEL_I, device="cuda", dtype=torch.int32),
               torch.full((total,), SENTINEL_I, device="cuda", dtype=torch.int32))
        o, g, b, c, status = ops.box_proposal_ar(*dev, ALL, limits, thr, item_off, overlap=buf[0], match_gt=buf[1], match_box=buf[2])
        assert int(status.item()) == 0
        outs.append((o.cpu().numpy().copy(), g.cpu().numpy().copy(), b.cpu().numpy().copy(), c.cpu().numpy().copy()))
    n = len(keep)
    got = outs[0]
    assert same_bits(got[0][:n][keep], ov) and np.array_equal(got[1][:n][keep], mg) and np.array_equal(got[2][:n][keep], mb)
    assert np.array_equal(got[3], cnt)
    assert (got[0][:n][~keep] == SENTINEL_F).all() and (got[1][:n][~keep] == SENTINEL_I).all() and (got[2][:n][~keep] == SENTINEL_I).all()
    assert (got[0][n:] == SENTINEL_F).all() and (got[1][n:] == SENTINEL_I).all() and (got[2][n:] == SENTINEL_I).all()
    for x, y in zip(outs[0], outs[1]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_misuse_is_refused_and_leaves_the_outputs_untouched(ops):
    from sos_wsod_amd._lib import HipKernelError
    rng = np.random.default_rng(8)
    images = [make_image(rng, 20, 5), make_image(rng, 10, 200)]
    lens, ov, _, _, _ = expected(images, ALL, (0,), (0.5,))
    dev, item_off = device_split(images, lens)

    def refused(exc, area_rng=ALL, limits=(0,), thr=(0.5,), dev=dev, item_off=item_off, status_code=None, **kw):
        whole, views = guarded(len(ov))
        if exc is not None:
            with pytest.raises(exc):
                ops.box_proposal_ar(*dev, area_rng, limits, thr, item_off, overlap=views[0], match_gt=views[1], match_box=views[2], **kw)
        else:
            status = ops.box_proposal_ar(*dev, area_rng, limits, thr, item_off, overlap=views[0], match_gt=views[1], match_box=views[2], **kw)[4]
            assert int(status.item()) == status_code
        return whole

    def untouched(whole):
        return all(bool((w == s).all()) for w, s in zip(whole, (SENTINEL_F, SENTINEL_I, SENTINEL_I)))

    assert untouched(refused(HipKernelError, area_rng=ALL * 9, item_off=torch.zeros(9 * 2 + 1, dtype=torch.int64, device="cuda")))       # A > 8
    assert untouched(refused(HipKernelError, limits=(0,) * 9, item_off=torch.zeros(9 * 2 + 1, dtype=torch.int64, device="cuda")))      # L > 8
    assert untouched(refused(HipKernelError, thr=[0.5] * 17))                                                                          # T > 16
    assert untouched(refused(HipKernelError, limits=(-1,)))                                                                            # negative limit
    assert untouched(refused(HipKernelError, item_off=item_off[:-1].contiguous()))                                                     # item_off too short
    bad = [t.clone() for t in dev]
    bad[0][1] = bad[0][2] + 1                                                                                                          # prop_off decreases
    assert untouched(refused(ValueError, dev=bad))
    bad = [t.clone() for t in dev]
    bad[2][1] = bad[2][2] + 3                                                                                                          # gt_off decreases
    assert untouched(refused(ValueError, dev=bad))
    # the kernel's own guards, with the wrapper's check off: the image or item is skipped and reported, never written
    assert untouched(refused(None, dev=bad, check_offsets=False, max_boxes=300, max_props=20, status_code=1))
    wrong = item_off.clone()
    wrong[1:] += 1                                                                                # regions of another split
    whole = refused(None, item_off=wrong, check_offsets=False, max_boxes=300, max_props=20, status_code=2)
    assert untouched(whole)
    # the second image needs the workspace (200 boxes); one sized for fewer is refused for that item, the first image is served
    whole = refused(None, max_boxes=150, max_props=20, status_code=3)
    n0 = int(lens[0])
    assert same_bits(whole[0][GUARD:GUARD + n0].cpu().numpy(), ov[:n0]) and bool((whole[0][GUARD + n0:] == SENTINEL_F).all())


# ------------------------------------------------------------------------------------------------------------------- evaluator
def test_evaluator_end_to_end_on_the_random_case(golden_dir, tmp_path):
    from sos_wsod_amd import evaluation as E
    z = F.load(golden_dir, "random")
    ds, preds, _ = F.case("random")
    js = tmp_path / "gt.json"
    js.write_text(json.dumps(ds))
    out_dir = tmp_path / "out"
    ev = E.COCOEvaluator(str(js), output_dir=str(out_dir), box_proposals=True)
    ev.reset()
    recs = F.records(preds)
    for k in range(0, len(recs), 8):
        ev.process([{"image_id": r["image_id"]} for r in recs[k:k + 8]], [{"proposals": r["proposals"].to("cuda")} for r in recs[k:k + 8]])
    res = ev.evaluate()
    assert list(res) == ["box_proposals"] and list(res["box_proposals"]) == list(F.EVALUATOR_KEYS)
    for (area, limit), key in zip(F.EVALUATOR_SETTINGS, F.EVALUATOR_KEYS):
        assert res["box_proposals"][key] == float(z[F.key(area, limit) + "/ar100"]), key
    with open(out_dir / "box_proposals.pkl", "rb") as f:
        raw = pickle.load(f)
    assert set(raw) == {"boxes", "objectness_logits", "ids", "bbox_mode"} and raw["ids"] == [p["image_id"] for p in preds]
    assert all(np.array_equal(b, p["boxes"]) for b, p in zip(raw["boxes"], preds))
    # the command line scores that file to the same numbers
    cli = E.main(["--proposals", str(out_dir / "box_proposals.pkl"), "--coco-json", str(js)])
    assert dict(cli["box_proposals"]) == dict(res["box_proposals"])


# ------------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def stage3w(golden_dir):
    """the detector of tests/golden/stage3_w.npz and a ProposalNetwork with its weights; the fixture's proposals were made with
    the training top-k (the teacher stays in training mode), so both eval-mode RPNs are given those counts"""
    from oracle import frcnn_oracle as FO
    from sos_wsod_amd.frcnn import ProposalNetwork
    from test_gpu_stage3 import _inputs, _Keys, _model
    t = np.load(os.path.join(golden_dir, "stage3_w.npz"))
    K = int(t["K"])
    det = _model(K, FO.make_params(K, tag="s3w", head_scale=float(t["head_scale"])), "s3w")
    topk = dict(pre_nms_topk=(det.proposal_generator.pre_nms_topk[0],) * 2, post_nms_topk=(det.proposal_generator.post_nms_topk[0],) * 2)
    det.proposal_generator.pre_nms_topk, det.proposal_generator.post_nms_topk = topk["pre_nms_topk"], topk["post_nms_topk"]
    pn = ProposalNetwork(sampler=_Keys("s3w"), rpn=topk).cuda()
    pn.load_detector_state_dict(det.state_dict())
    return t, K, det, pn, _inputs


def test_proposal_network_gives_the_detectors_proposals(stage3w):
    from test_gpu_stage3 import _same_boxes          # the bar that test applies to prop_boxes* of this fixture (it sets none for prop_logits*)
    t, K, det, pn, _inputs = stage3w
    det.eval(); pn.eval()
    data, _ = _inputs("s3w", t, K, with_gt=False)
    raw = pn.inference(data, do_postprocess=False)
    with torch.no_grad():
        det.refresh_staged_weights()
        x4, sizes = det.preprocess_image(data)
        want, _ = det.proposal_generator(sizes, det._features(x4), None, compute_loss=False)
    assert len(raw) == len(want) == 2
    for i, (a, b) in enumerate(zip(raw, want)):
        assert torch.equal(a.proposal_boxes.tensor, b.proposal_boxes.tensor) and torch.equal(a.objectness_logits, b.objectness_logits)
        assert _same_boxes(a.proposal_boxes.tensor.cpu().numpy(), t[f"prop_boxes{i}"])
    # after postprocessing to another output size: the restatement of modeling/postprocessing.py
    for d, (h, w) in zip(data, ((333, 517), (480, 251))):
        d["height"], d["width"] = h, w
    out = pn(data)
    for o, a, d in zip(out, raw, data):
        assert set(o) == {"proposals"}
        wb, wl = R.postprocess_proposals(a.proposal_boxes.tensor.cpu().numpy(), a.objectness_logits.cpu().numpy(), a.image_size,
                                         d["height"], d["width"])
        got = o["proposals"]
        assert got.image_size == (d["height"], d["width"])
        assert np.array_equal(got.proposal_boxes.tensor.cpu().numpy().view(np.uint32), wb.view(np.uint32))
        assert np.array_equal(got.objectness_logits.cpu().numpy(), wl)


def test_proposal_network_trains_on_the_two_rpn_losses(stage3w):
    from test_gpu_stage3 import _Keys
    t, K, det, pn, _inputs = stage3w
    data, _ = _inputs("s3w", t, K, with_gt=True)
    det.train(); pn.train()
    for m in (det, pn):                                            # the same sampling keys for both
        m.sampler = m.proposal_generator.sampler = _Keys("s3w-train")
    det.roi_heads.sampler = det.sampler
    want = det(data, branch="supervised")[0]
    got = pn(data)
    assert set(got) == {"loss_rpn_cls", "loss_rpn_loc"}
    for k in got:
        assert torch.equal(got[k].detach(), want[k].detach()), k
    sum(got.values()).backward()
    assert pn.proposal_generator.rpn_head.conv.weight.grad is not None
