"""Read image files into planar uint8 device tensors, pixels equal to Pillow's: the package's stand-in for the reference's
detection_utils.read_image (detectron2/data/detection_utils.py:119-185: Image.open, the EXIF orientation, convert("RGB"), the plane
reversal for BGR).

A baseline JPEG is decoded in two halves.  The host parses the markers and undoes the Huffman coding (csrc/jpeg.hip's plain C++
part, run on a thread pool: ctypes drops the GIL) into pinned memory; one copy carries the quantised coefficients of a whole batch
to the device; two kernels (sw_jpeg_decode_batch) dequantise, run libjpeg's integer IDCT, upsample the chroma, convert the colour
and write the planes in the order asked.  The EXIF orientation is then an exact torch flip / transpose.

What the decoder does not cover (progressive, CMYK, unusual samplings, ...; ops.jpeg_probe returns 0) and files that are not JPEG
at all are decoded by Pillow on the host, as the reference does, and uploaded; `return_paths=True` says which way each image went.
A malformed JPEG stream raises ValueError with the host code's reason.
"""
import ctypes
import io
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops
from ._lib import JpegDesc, JpegInfo

MAX_THREADS = 16                       # never sized by os.cpu_count(): a job is given a share of the machine, not all of it
_FORMATS = ("RGB", "BGR")
_pools = {}


def _pool(threads):
    p = _pools.get(threads)
    if p is None:
        p = _pools[threads] = ThreadPoolExecutor(threads, thread_name_prefix="sw_jpeg")
    return p


def _as_bytes(src):
    """path, bytes-like or uint8 array -> contiguous 1-D uint8 numpy array"""
    if isinstance(src, (str, os.PathLike)):
        return np.fromfile(src, dtype=np.uint8)
    if isinstance(src, (bytes, bytearray, memoryview)):
        return np.frombuffer(src, dtype=np.uint8)
    if torch.is_tensor(src):
        src = src.cpu().numpy()
    a = np.asarray(src)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise TypeError("an image source is a path, bytes or a 1-D uint8 array")
    return np.ascontiguousarray(a)


def _check_format(format):
    if format not in _FORMATS:
        raise ValueError(f"format {format!r} is not implemented: one of {_FORMATS}")


def _device(device):
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("sos-wsod_amd kernels need a GPU device (there is no CPU pixel path)")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


def apply_orientation(img, orientation):
    """(3, H, W) tensor -> what Image.transpose gives for that EXIF orientation (detection_utils._apply_exif_orientation): 2
    FLIP_LEFT_RIGHT, 3 ROTATE_180, 4 FLIP_TOP_BOTTOM, 5 TRANSPOSE, 6 ROTATE_270, 7 TRANSVERSE, 8 ROTATE_90; anything else: as is"""
    if orientation == 2:
        img = img.flip(2)
    elif orientation == 3:
        img = img.flip(1, 2)
    elif orientation == 4:
        img = img.flip(1)
    elif orientation == 5:
        img = img.transpose(1, 2)
    elif orientation == 6:
        img = img.transpose(1, 2).flip(2)
    elif orientation == 7:
        img = img.transpose(1, 2).flip(1, 2)
    elif orientation == 8:
        img = img.transpose(1, 2).flip(1)
    else:
        return img
    return img.contiguous()


def probe(src):
    """-> (code, JpegInfo) of ops.jpeg_probe for a path, bytes or uint8 array"""
    return ops.jpeg_probe(_as_bytes(src))


def _round256(n):
    return (n + 255) // 256 * 256


def decode_batch(datas, infos, format="BGR", device=None, threads=None, outs=None, workspace=None):
    """The device path alone, before the EXIF orientation: datas are uint8 arrays, infos the JpegInfo of each (probe code 1).
    Host entropy decode on min(16, n) threads into one pinned buffer, ONE upload, ONE sw_jpeg_decode_batch call.
    outs: (3, H, W) uint8 device tensors to write (default: new ones); workspace: a uint8 device tensor of at least
    ops.jpeg_workspace_bytes bytes starting on a 256-byte boundary (default: a new one).  -> outs"""
    _check_format(format)
    dev = _device(device)
    n = len(datas)
    if n == 0:
        return []
    arr = (JpegInfo * n)(*infos)
    ws_bytes = ops.jpeg_workspace_bytes(arr)
    o_desc, o_qtab = 0, _round256(n * ctypes.sizeof(JpegDesc))
    o_coef = o_qtab + _round256(n * 512)
    coef_off = np.concatenate([[0], np.cumsum([f.coef_bytes for f in infos])]).astype(np.int64)
    stage = torch.empty(o_coef + int(coef_off[-1]), dtype=torch.uint8, pin_memory=True)
    host = stage.data_ptr()

    def work(i):
        return ops.jpeg_entropy_decode(datas[i], arr[i], host + o_coef + int(coef_off[i]), host + o_qtab + 512 * i)

    threads = min(MAX_THREADS, n) if threads is None else max(1, min(int(threads), MAX_THREADS, n))
    codes = [work(i) for i in range(n)] if threads == 1 else list(_pool(threads).map(work, range(n)))
    for i, rc in enumerate(codes):
        if rc != 0:
            raise ValueError(f"image {i} of the batch: malformed JPEG stream: {ops.jpeg_error(rc)} (code {rc})")
    with torch.cuda.device(dev):
        if outs is None:
            outs = [torch.empty((3, f.height, f.width), dtype=torch.uint8, device=dev) for f in infos]
        if workspace is None:
            workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        ops._need_gpu(workspace)
        if workspace.dtype != torch.uint8 or workspace.numel() < ws_bytes or workspace.data_ptr() % 256 or not workspace.is_contiguous():
            raise ValueError(f"workspace: a contiguous uint8 tensor of >= {ws_bytes} bytes on a 256-byte boundary")
        total_blocks, total_quads = ops.jpeg_describe_batch(arr, outs, format == "BGR", host + o_desc)
        staged = stage.to(dev, non_blocking=True)
        base = staged.data_ptr()
        ops.jpeg_decode_batch(n, base + o_desc, total_blocks, total_quads, base + o_coef, base + o_qtab, workspace.data_ptr())
        # the launches are queued on the current stream; the caching allocator keeps `staged` and `workspace` alive for them
    return outs


def _exif_orientation_pil(image):
    try:
        exif = image.getexif()
    except Exception:                                   # as the reference does (detection_utils.py:141-144)
        return 1
    return 1 if exif is None else exif.get(274, 1)


def _pillow_decode(data, format):
    """the reference's read_image on the host: -> ((3, H, W) uint8 CPU tensor, already oriented)"""
    from PIL import Image
    with Image.open(io.BytesIO(data.tobytes())) as im:
        o = _exif_orientation_pil(im)
        method = {2: Image.FLIP_LEFT_RIGHT, 3: Image.ROTATE_180, 4: Image.FLIP_TOP_BOTTOM, 5: Image.TRANSPOSE,
                  6: Image.ROTATE_270, 7: Image.TRANSVERSE, 8: Image.ROTATE_90}.get(o)
        if method is not None:
            im = im.transpose(method)
        a = np.asarray(im.convert("RGB"))
    if format == "BGR":
        a = a[:, :, ::-1]
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


def read_images(srcs, format="BGR", device=None, threads=None, return_paths=False):
    """A batch of image files -> list of (3, H, W) uint8 device tensors, planes in `format` order ("RGB" or "BGR"), pixels equal to
    detection_utils.read_image's.  srcs: paths, bytes or uint8 arrays, of any mix of sizes and samplings.  threads: host decode
    threads (default min(16, len(srcs))).  return_paths: also the list of "device" / "pillow", which decoder each image took."""
    _check_format(format)
    dev = _device(device)
    datas = [_as_bytes(s) for s in srcs]
    covered, infos, paths = [], [], []
    for i, d in enumerate(datas):
        rc, info = ops.jpeg_probe(d)
        if rc == 1:
            covered.append(i)
            infos.append(info)
        elif rc not in (0, -2):
            raise ValueError(f"image {i} of the batch: malformed JPEG stream: {ops.jpeg_error(rc)} (code {rc})")
        paths.append("device" if rc == 1 else "pillow")
    result = [None] * len(datas)
    decoded = decode_batch([datas[i] for i in covered], infos, format, dev, threads)
    for i, f, t in zip(covered, infos, decoded):
        result[i] = apply_orientation(t, f.orientation)
    for i, d in enumerate(datas):
        if result[i] is None:
            result[i] = _pillow_decode(d, format).to(dev)
    return (result, paths) if return_paths else result


def read_image(src, format="BGR", device=None, return_path=False):
    """One image file -> (3, H, W) uint8 device tensor: read_images of one source, host decode on the calling thread"""
    out, paths = read_images([src], format, device, threads=1, return_paths=True)
    return (out[0], paths[0]) if return_path else out[0]


class JpegLoader:
    """`image_loader` of split.score_images and strong_aug.TwoCropBatches: dataset dict -> read_image(d["file_name"])"""

    def __init__(self, format="BGR", device=None):
        _check_format(format)
        self.format, self.device = format, device

    def __call__(self, d):
        return read_image(d["file_name"], self.format, self.device)
