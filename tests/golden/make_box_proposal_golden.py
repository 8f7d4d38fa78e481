"""Generate tests/golden/box_proposal_{hand,random,coco}.npz by RUNNING the reference's `_evaluate_box_proposals`
(detectron2/detectron2/evaluation/coco_evaluation.py:427-535) from its place in the reference tree — build container only:

    python tests/golden/make_box_proposal_golden.py [OUT_DIR]          (default OUT_DIR: tests/golden)

The file is loaded under ref_shim_d2.install() (the reference's own Boxes, BoxMode, pairwise_iou and Instances), with stub modules
for what it imports at its top and this function never touches: pycocotools.*, tabulate, detectron2.config.CfgNode,
detectron2.data.MetadataCatalog, detectron2.data.datasets.coco, detectron2.evaluation.fast_eval_api / .evaluator,
detectron2.utils.file_io.PathManager, detectron2.utils.logger.create_small_table.  `coco_api` is a two-method stand-in
(getAnnIds / loadAnns over the fixture's annotation list, as pycocotools' imgToAnns gives them: every annotation of the image, in
file order).  The inputs come from tests/box_proposal_fixture.py; stored per (area, limit): the reference's gt_overlaps, recalls,
ar and num_pos, and the SHA-256 of the inputs.  Run it in its own process (ref_shim_d2's module names collide with ref_shim's)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import box_proposal_fixture as F  # noqa: E402
import ref_shim_d2 as S  # noqa: E402


class FakeCOCO:
    def __init__(self, ds):
        self.anns = {a["id"]: a for a in ds["annotations"]}
        self.by_img = {}
        for a in ds["annotations"]:
            self.by_img.setdefault(a["image_id"], []).append(a["id"])

    def getAnnIds(self, imgIds):
        return list(self.by_img.get(imgIds, []))

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]


def load_reference():
    ns = S.install()
    for name, attrs in (("pycocotools", {}), ("pycocotools.mask", {}), ("pycocotools.coco", {"COCO": None}),
                        ("pycocotools.cocoeval", {"COCOeval": None}), ("tabulate", {"tabulate": None}),
                        ("detectron2.data.datasets", {}), ("detectron2.data.datasets.coco", {"convert_to_coco_json": None}),
                        ("detectron2.evaluation", {}), ("detectron2.evaluation.fast_eval_api", {"COCOeval_opt": None}),
                        ("detectron2.evaluation.evaluator", {"DatasetEvaluator": object})):
        m = S._pkg(name, S.D2 + "/evaluation" if name == "detectron2.evaluation" else None)
        for k, v in attrs.items():
            setattr(m, k, v)
    sys.modules["detectron2.config"].CfgNode = type("CfgNode", (), {})
    sys.modules["detectron2.data"].MetadataCatalog = None
    sys.modules["detectron2.utils.logger"].create_small_table = None
    ev = S._load("detectron2.evaluation.coco_evaluation", S.D2 + "/evaluation/coco_evaluation.py")
    return ns, ev


def main(out_dir):
    ns, ev = load_reference()
    for name in F.CASES:
        ds, preds, settings = F.case(name)
        api = FakeCOCO(ds)
        dataset_predictions = []
        for p in preds:
            inst = ns.instances.Instances((480, 640))
            inst.proposal_boxes = ns.boxes.Boxes(torch.from_numpy(p["boxes"].copy()))
            inst.objectness_logits = torch.from_numpy(p["logits"].copy())
            dataset_predictions.append({"image_id": p["image_id"], "proposals": inst})
        z = {"sha256": np.asarray(F.inputs_sha256(ds, preds))}
        for area, limit in settings:
            stats = ev._evaluate_box_proposals(dataset_predictions, api, area=area, limit=limit)
            k = F.key(area, limit)
            assert stats["gt_overlaps"].dtype == torch.float32 and stats["recalls"].dtype == torch.float32
            z[k + "/gt_overlaps"] = stats["gt_overlaps"].numpy()
            z[k + "/recalls"] = stats["recalls"].numpy()
            z[k + "/ar"] = np.asarray(stats["ar"].item(), dtype=np.float32)
            z[k + "/ar100"] = np.asarray(float(stats["ar"].item() * 100), dtype=np.float64)      # :290, the evaluator's number
            z[k + "/num_pos"] = np.asarray(stats["num_pos"], dtype=np.int64)
        path = os.path.join(out_dir, f"box_proposal_{name}.npz")
        np.savez_compressed(path, **z)
        print(path, os.path.getsize(path), "bytes;", len(preds), "predictions,", len(ds["annotations"]), "annotations;",
              {F.key(a, l): round(float(z[F.key(a, l) + "/ar"]), 4) for a, l in settings[:4]})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
