"""Cost of reading JPEG files into device tensors: image_io.read_images (Huffman decoding on host threads, one upload, two kernels)
against the path every caller had to write before it, which is split._pillow_bgr's: Pillow decode + convert("RGB") + plane
reversal + upload, on the same number of host threads (Pillow drops the GIL while it decodes).

Workload: 64 different 500 x 375 files, 4:2:0, quality 90, synthetic low-pass noise (a VOC-sized photograph's statistics, roughly;
no dataset is needed).  For host threads 1, 4, 16 and batches of 1, 8, 64: images/s of both paths, each figure the median of
--repeats passes of --rounds times all 64 files (512 decodes, 35 ms to 0.4 s per pass), the two paths alternating, every pass ending
in a device synchronise, after a warm-up pass of each.
Then the two kernels alone on a staged batch of 64 (HIP events around --iters calls): time per image, the bytes they move by
construction (coefficients in, planes out; planes in, pixels out) and that traffic as a share of the 8 TB/s HBM peak.
-> one JSON line (and --out FILE).

    python tools/jpeg_decode_bench.py [--repeats 7] [--rounds 8] [--iters 200] [--out FILE]

Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/jpeg_decode_bench.py --kernels-only --iters 50` (jpeg_idct_kernel, jpeg_pixel_kernel)."""
import argparse
import ctypes
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
N_FILES, W, H = 64, 500, 375
THREADS, BATCHES = (1, 4, 16), (1, 8, 64)


def make_files():
    from PIL import Image
    g = np.random.default_rng(0)
    files = []
    for _ in range(N_FILES):
        low = Image.fromarray(g.integers(0, 256, (H // 12 + 2, W // 12 + 2, 3), dtype=np.uint8), "RGB").resize((W, H), Image.BICUBIC)
        a = np.asarray(low).astype(np.int16) + g.integers(-6, 7, (H, W, 3), dtype=np.int16)
        buf = io.BytesIO()
        Image.fromarray(a.clip(0, 255).astype(np.uint8), "RGB").save(buf, "JPEG", quality=90, subsampling=2)
        files.append(np.frombuffer(buf.getvalue(), np.uint8))
    return files


def pillow_bgr(data):
    """split._pillow_bgr from memory: decode, convert("RGB"), reverse the planes"""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        a = np.asarray(im.convert("RGB"))
    return torch.from_numpy(np.ascontiguousarray(a[:, :, ::-1].transpose(2, 0, 1)))


def timed_pass(fn, batches, rounds):
    """fn(batch) -> device tensors.  -> a function that runs every batch `rounds` times, synchronises and returns the seconds it took"""
    def one_pass():
        t0 = time.perf_counter()
        for _ in range(rounds):
            for b in batches:
                fn(b)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    return one_pass


def kernels_alone(files, iters):
    """-> (ms per call of the two launches for all files as one batch, bytes moved per image by each kernel, coefficient bytes per image)"""
    import sos_wsod_amd.ops as ops
    from sos_wsod_amd._lib import JpegDesc, JpegInfo
    infos = [ops.jpeg_probe(d)[1] for d in files]
    n = len(files)
    arr = (JpegInfo * n)(*infos)
    r256 = lambda v: (v + 255) // 256 * 256
    o_q = r256(n * ctypes.sizeof(JpegDesc))
    o_c = o_q + r256(n * 512)
    offs = np.concatenate([[0], np.cumsum([f.coef_bytes for f in infos])])
    stage = torch.empty(o_c + int(offs[-1]), dtype=torch.uint8, pin_memory=True)
    for i, d in enumerate(files):
        assert ops.jpeg_entropy_decode(d, arr[i], stage.data_ptr() + o_c + int(offs[i]), stage.data_ptr() + o_q + 512 * i) == 0
    outs = [torch.empty((3, f.height, f.width), dtype=torch.uint8, device="cuda") for f in infos]
    ws = torch.empty(ops.jpeg_workspace_bytes(arr), dtype=torch.uint8, device="cuda")
    tb, tq = ops.jpeg_describe_batch(arr, outs, True, stage.data_ptr())
    dev = stage.cuda()
    run = lambda: ops.jpeg_decode_batch(n, dev.data_ptr(), tb, tq, dev.data_ptr() + o_c, dev.data_ptr() + o_q, ws.data_ptr())
    for _ in range(10):
        run()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        run()
    b.record()
    torch.cuda.synchronize()
    blocks = sum(f.coef_bytes // 128 for f in infos) / n
    return a.elapsed_time(b) / iters, {"idct": 128 * blocks + 64 * blocks, "pixel": 64 * blocks + 3 * H * W}, int(offs[-1]) // n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=8, help="a timed pass goes over the 64 files this many times")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kernels-only", action="store_true", help="only the two kernels on a staged batch (profiling runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import sos_wsod_amd  # noqa: F401
    from sos_wsod_amd.image_io import read_images
    assert torch.cuda.is_available(), "this benchmark measures the GPU path; there is no fallback"
    files = make_files()
    raw = [f.tobytes() for f in files]
    ms, moved, coef_bytes = kernels_alone(files, args.iters)
    per_image_us = ms * 1e3 / N_FILES
    res = {"workload": {"files": N_FILES, "wh": [W, H], "sampling": "4:2:0", "quality": 90, "decodes_per_timed_pass": N_FILES * args.rounds, "repeats": args.repeats,
                        "mean_file_bytes": int(np.mean([f.size for f in files])), "coefficient_bytes_uploaded_per_image": coef_bytes,
                        "decoded_bytes_per_image": 3 * H * W},
           "kernels": {"both_launches_ms_per_batch_of_64_events": round(ms, 4), "both_kernels_us_per_image": round(per_image_us, 3),
                       "bytes_moved_per_image": {k: int(v) for k, v in moved.items()},
                       "traffic_over_event_time_share_of_hbm_peak": round(sum(moved.values()) * N_FILES / (ms * 1e-3) / HBM_PEAK, 4)}}
    if not args.kernels_only:
        table = []
        for t in THREADS:
            pool = ThreadPoolExecutor(t) if t > 1 else None
            for bs in BATCHES:
                idx = [list(range(s, min(s + bs, N_FILES))) for s in range(0, N_FILES, bs)]
                dev_fn = lambda b: read_images([files[i] for i in b], "BGR", threads=t)
                if pool is None:
                    pil_fn = lambda b: [pillow_bgr(raw[i]).cuda(non_blocking=True) for i in b]
                else:
                    pil_fn = lambda b: [x.cuda(non_blocking=True) for x in pool.map(pillow_bgr, [raw[i] for i in b])]
                passes = {"device": timed_pass(dev_fn, idx, args.rounds), "pillow": timed_pass(pil_fn, idx, args.rounds)}
                for p in passes.values():                                      # warm-up: pools, pinned buffers, code objects
                    p()
                times = {k: [] for k in passes}
                for _ in range(args.repeats):                                  # alternating
                    for k, p in passes.items():
                        times[k].append(p())
                row, n_img = {"threads": t, "batch": bs}, N_FILES * args.rounds
                for k, v in times.items():
                    row[k + "_images_per_s"] = round(n_img / statistics.median(v), 1)
                    row[k + "_spread"] = [round(n_img / max(v), 1), round(n_img / min(v), 1)]
                row["device_over_pillow"] = round(row["device_images_per_s"] / row["pillow_images_per_s"], 3)
                table.append(row)
                print(row, file=sys.stderr, flush=True)
            if pool is not None:
                pool.shutdown()
        res["read_images_vs_pillow"] = table
        a = read_images(files[:8], "BGR")
        assert all(torch.equal(x.cpu(), pillow_bgr(raw[i])) for i, x in enumerate(a)), "the two paths disagree"
        res["pixels_equal_on_the_workload"] = True
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
