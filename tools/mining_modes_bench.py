"""The mining kernels under OICRPlusHeads' other rules: sw_oicr_mine_label in its default form (top-p% + threshold + NMS), its top-1
form (WSL.REFINE_MIST False) and its candidate-box form (OICRPLUS.BBOX_UPDATE True), and sw_oicr_update_boxes — 4 refinement rounds
per launch as the step launches them, median of 31 launches each — then the full training step with BBOX_UPDATE off and on."""
import os, sys, time, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench
import sos_wsod_amd.ops as ops
from sos_wsod_amd.inference import SCALE_CLAMP
from sos_wsod_amd.solver import HipSGD
from sos_wsod_amd.trainer import Trainer
dev = "cuda"
N = 31


def median_us(fn):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(N):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return sorted(ts)[N // 2]


def kernels(R, K, G, rounds=4, V=4):
    g = torch.Generator().manual_seed(0)
    x1 = torch.rand(R, generator=g) * 480; y1 = torch.rand(R, generator=g) * 480
    boxes = torch.stack([x1, y1, x1 + 24 + torch.rand(R, generator=g) * 200, y1 + 24 + torch.rand(R, generator=g) * 200], 1).to(dev)
    scores = torch.softmax(torch.randn(rounds, R, K + 1, generator=g), -1).to(dev)
    gt = torch.randperm(K, generator=g)[:G].sort().values.int().to(dev)
    stride = 5 * K + 1
    logits = torch.randn(V * R, rounds * stride, generator=g).to(dev)
    signs = torch.tensor([1, -1, 1, -1], dtype=torch.int32, device=dev)
    cand = torch.empty(rounds - 1, R, G, 4, device=dev)
    i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
    f32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)

    def mine(top_k, **kw):
        n = top_k * G
        out = (i32(rounds, R), f32(rounds, R), i32(rounds, R), i32(rounds), i32(rounds, n), i32(rounds, n), f32(rounds, n))
        ws = torch.empty(ops.mine_workspace_bytes(R, top_k, G, rounds), device=dev, dtype=torch.uint8)
        if kw:
            kw = dict(kw, lab_box=f32(rounds, R, 4), pgt_box=f32(rounds, n, 4))
        return median_us(lambda: ops.oicr_mine_label(scores, gt, boxes, K, top_k, 0.05, 0.01, 0.5, 0.6, *out, ws, **kw)), out[3].tolist()
    top_k = max(int(R * 0.10), 1)
    decode = lambda: ops.oicr_update_boxes(logits, V, R, K, rounds - 1, K + 1, stride, boxes, gt, signs, (10.0, 10.0, 5.0, 5.0), SCALE_CLAMP, cand)
    t_dec = median_us(decode)
    t0, k0 = mine(top_k)
    t1, k1 = mine(1, seed_rule=1)
    t2, k2 = mine(top_k, cand_boxes=cand, cand_from=1, seed_rule=0)
    t3, k3 = mine(top_k, seed_rule=0, cand_boxes=None)          # the extended instantiation on proposal boxes: lab_box / pgt_box only
    print(f"R={R} K={K} G={G}: mine_label default {t0:.0f} us (kept {k0}) | top-1 {t1:.0f} us | candidate boxes {t2:.0f} us (kept {k2}) | "
          f"extended, proposal boxes {t3:.0f} us | update_boxes {t_dec:.1f} us")


def step(bbox_update, refine_mist=True):
    d = torch.device("cuda", 0)
    model = bench.build(d, torch.bfloat16); model.train()
    model.roi_heads.bbox_update, model.roi_heads.refine_mist = bbox_update, refine_mist
    opt = HipSGD([{"params": [p], "lr": 1e-3, "weight_decay": 5e-4} for p in model.parameters() if p.requires_grad], 1e-3, momentum=0.9)
    tr = Trainer(model, opt)
    data = bench.make_inputs(d, 1)
    for _ in range(5): tr.run_step(data)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(20): tr.run_step(data)
    torch.cuda.synchronize()
    print(f"step R={bench.R} BBOX_UPDATE={bbox_update} REFINE_MIST={refine_mist}: {(time.perf_counter() - t0) * 50:.3f} ms/step")


kernels(2000, 20, 2); kernels(4000, 20, 5)
step(False); step(True); step(False, refine_mist=False)
