"""NumPy restatement of the baseline JPEG decode chain as libjpeg runs it for Pillow: marker parser, Huffman decoding,
dequantisation, the "islow" integer inverse DCT, "fancy" chroma upsampling and the fixed-point YCbCr -> RGB conversion.  Written
from the public description of the format (ITU-T T.81, JFIF, the EXIF TIFF layout) and of libjpeg's arithmetic; slow and plain on
purpose.  tests/test_jpeg_ref_cpu.py pins it to Pillow's pixels; the C host code and the HIP kernels are then compared with it
stage by stage.

Status of parse(): 1 = covered by the package's decoder, 0 = a valid-looking file it leaves to Pillow; MalformedJpeg otherwise.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])


class MalformedJpeg(ValueError):
    pass


def _u16(b, i):
    return (b[i] << 8) | b[i + 1]


def _exif_orientation(seg):
    """seg: the APP1 payload after its length.  -> tag 274 of IFD0, or None"""
    if len(seg) < 14 or bytes(seg[:6]) != b"Exif\0\0":
        return None
    t = bytes(seg[6:])
    if t[:4] == b"II*\0":
        rd = lambda o, n: int.from_bytes(t[o:o + n], "little")
    elif t[:4] == b"MM\0*":
        rd = lambda o, n: int.from_bytes(t[o:o + n], "big")
    else:
        return None
    ifd = rd(4, 4)
    if ifd + 2 > len(t):
        return None
    for k in range(rd(ifd, 2)):
        e = ifd + 2 + 12 * k
        if e + 12 > len(t):
            return None
        if rd(e, 2) == 274:
            typ = rd(e + 2, 2)
            if typ == 3:
                return rd(e + 8, 2)
            if typ == 4:
                return rd(e + 8, 4)
            return None
    return None


def parse(data):
    """-> dict(status, width, height, ncomp, hs, vs, tq, restart, orientation, blocks_w, blocks_h, mcus_x, mcus_y, q (4, 64) natural
    order, huff {(class, id): (bits[16], values)}, td, ta, scan (offset of the entropy-coded bytes))"""
    b = bytes(data)
    n = len(b)
    if n < 4 or b[0] != 0xFF or b[1] != 0xD8:
        raise MalformedJpeg("no SOI")
    p = dict(status=1, restart=0, orientation=1, q=np.zeros((4, 64), np.uint16), qdef=[False] * 4, huff={}, sof=None)
    jfif = False
    adobe = None
    exif_seen = False
    i = 2
    while True:
        if i >= n:
            raise MalformedJpeg("truncated")
        if b[i] != 0xFF:
            raise MalformedJpeg("marker expected")
        while i < n and b[i] == 0xFF:
            i += 1
        if i >= n:
            raise MalformedJpeg("truncated")
        m = b[i]
        i += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9 or m == 0xD8 or m == 0:
            raise MalformedJpeg("unexpected marker")
        if i + 2 > n:
            raise MalformedJpeg("truncated")
        L = _u16(b, i)
        if L < 2 or i + L > n:
            raise MalformedJpeg("bad segment length")
        seg = b[i + 2:i + L]
        if m in (0xC0, 0xC1):
            if p["sof"] is not None:
                raise MalformedJpeg("two frames")
            if len(seg) < 6:
                raise MalformedJpeg("short SOF")
            prec, h, w, nc = seg[0], _u16(seg, 1), _u16(seg, 3), seg[5]
            if len(seg) != 6 + 3 * nc:
                raise MalformedJpeg("bad SOF length")
            if prec not in (8, 12) or w == 0 or nc == 0:
                raise MalformedJpeg("bad SOF")
            p.update(sof=m, precision=prec, width=w, height=h, ncomp=nc, cid=[seg[6 + 3 * c] for c in range(nc)],
                     hs=[seg[7 + 3 * c] >> 4 for c in range(nc)], vs=[seg[7 + 3 * c] & 15 for c in range(nc)],
                     tq=[seg[8 + 3 * c] for c in range(nc)])
            if any(not (1 <= x <= 4) for x in p["hs"] + p["vs"]) or any(t > 3 for t in p["tq"]):
                raise MalformedJpeg("bad SOF component")
        elif 0xC2 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            p["status"] = 0                                   # progressive, lossless, arithmetic, hierarchical
            return p
        elif m == 0xC4:
            j = 0
            while j < len(seg):
                if j + 17 > len(seg):
                    raise MalformedJpeg("short DHT")
                tc, th = seg[j] >> 4, seg[j] & 15
                bits = list(seg[j + 1:j + 17])
                cnt = sum(bits)
                if tc > 1 or th > 3 or cnt > 256 or j + 17 + cnt > len(seg):
                    raise MalformedJpeg("bad DHT")
                code = 0
                for ln in range(16):
                    code += bits[ln]
                    if code > (1 << (ln + 1)):
                        raise MalformedJpeg("bad DHT counts")
                    code <<= 1
                p["huff"][(tc, th)] = (bits, list(seg[j + 17:j + 17 + cnt]))
                j += 17 + cnt
        elif m == 0xDB:
            j = 0
            while j < len(seg):
                pq, tq = seg[j] >> 4, seg[j] & 15
                sz = 128 if pq else 64
                if pq > 1 or tq > 3 or j + 1 + sz > len(seg):
                    raise MalformedJpeg("bad DQT")
                for k in range(64):
                    p["q"][tq, ZIGZAG[k]] = _u16(seg, j + 1 + 2 * k) if pq else seg[j + 1 + k]
                p["qdef"][tq] = True
                j += 1 + sz
        elif m == 0xDD:
            if len(seg) != 2:
                raise MalformedJpeg("bad DRI")
            p["restart"] = _u16(seg, 0)
        elif m == 0xE0 and seg[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xE1 and seg[:6] == b"Exif\0\0" and not exif_seen:
            exif_seen = True
            o = _exif_orientation(seg)
            p["orientation"] = o if o is not None and 1 <= o <= 8 else 1
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif m == 0xDA:
            if p["sof"] is None:
                raise MalformedJpeg("SOS before SOF")
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
                raise MalformedJpeg("bad SOS")
            ns = seg[0]
            nc = p["ncomp"]
            if p["precision"] != 8 or p["height"] == 0 or nc not in (1, 3) or ns != nc:
                p["status"] = 0
                return p
            if [seg[1 + 2 * c] for c in range(nc)] != p["cid"]:
                raise MalformedJpeg("scan components out of order")
            p["td"] = [seg[2 + 2 * c] >> 4 for c in range(nc)]
            p["ta"] = [seg[2 + 2 * c] & 15 for c in range(nc)]
            if seg[1 + 2 * nc] != 0 or seg[2 + 2 * nc] != 63 or seg[3 + 2 * nc] != 0:
                raise MalformedJpeg("bad spectral selection")
            if nc == 1:
                if (p["hs"][0], p["vs"][0]) != (1, 1):
                    p["status"] = 0
                    return p
            else:
                if (p["hs"][0], p["vs"][0]) not in ((1, 1), (2, 1), (2, 2)) or p["hs"][1:] != [1, 1] or p["vs"][1:] != [1, 1]:
                    p["status"] = 0
                    return p
                if adobe is not None:
                    if adobe != 1:
                        p["status"] = 0
                        return p
                elif not jfif and p["cid"] == [82, 71, 66]:
                    p["status"] = 0
                    return p
            for c in range(nc):
                if not p["qdef"][p["tq"][c]]:
                    raise MalformedJpeg("missing quantisation table")
                if max(p["td"][c], p["ta"][c]) > 3 or (0, p["td"][c]) not in p["huff"] or (1, p["ta"][c]) not in p["huff"]:
                    raise MalformedJpeg("missing Huffman table")
            H, V = p["hs"][0], p["vs"][0]
            p["mcus_x"] = -(-p["width"] // (8 * H))
            p["mcus_y"] = -(-p["height"] // (8 * V))
            p["blocks_w"] = [p["mcus_x"] * p["hs"][c] for c in range(nc)]
            p["blocks_h"] = [p["mcus_y"] * p["vs"][c] for c in range(nc)]
            p["coef_bytes"] = 128 * sum(a * c for a, c in zip(p["blocks_w"], p["blocks_h"]))
            p["scan"] = i + L
            return p
        i += L


class _Bits:
    def __init__(self, b, pos):
        self.b, self.pos, self.acc, self.cnt, self.marker = b, pos, 0, 0, None

    def _byte(self):
        b = self.b
        if self.marker is not None:
            raise MalformedJpeg("entropy data ends early")
        if self.pos >= len(b):
            raise MalformedJpeg("truncated entropy data")
        v = b[self.pos]
        self.pos += 1
        if v == 0xFF:
            while self.pos < len(b) and b[self.pos] == 0xFF:
                self.pos += 1
            if self.pos >= len(b):
                raise MalformedJpeg("truncated entropy data")
            c = b[self.pos]
            self.pos += 1
            if c != 0:
                self.marker = c
                raise MalformedJpeg("entropy data ends early")
        return v

    def get(self, k):
        while self.cnt < k:
            self.acc = (self.acc << 8) | self._byte()
            self.cnt += 8
        self.cnt -= k
        v = (self.acc >> self.cnt) & ((1 << k) - 1)
        self.acc &= (1 << self.cnt) - 1
        return v

    def restart(self, expect):
        """drop the padding bits, read the RSTn marker"""
        if self.cnt >= 8:
            raise MalformedJpeg("data before the restart marker")
        self.acc = self.cnt = 0
        b = self.b
        if self.pos >= len(b) or b[self.pos] != 0xFF:
            raise MalformedJpeg("restart marker missing")
        while self.pos < len(b) and b[self.pos] == 0xFF:
            self.pos += 1
        if self.pos >= len(b) or b[self.pos] != expect:
            raise MalformedJpeg("restart marker missing")
        self.pos += 1


def _code_table(bits, vals):
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[(ln, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


def _symbol(br, table):
    code = 0
    for ln in range(1, 17):
        code = (code << 1) | br.get(1)
        s = table.get((ln, code))
        if s is not None:
            return s
    raise MalformedJpeg("bad Huffman code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def entropy_decode(p, data):
    """-> ([per component (blocks_h, blocks_w, 64) int16, natural order], the (4, 64) uint16 tables in natural order)"""
    assert p["status"] == 1
    b = bytes(data)
    nc = p["ncomp"]
    coef = [np.zeros((p["blocks_h"][c], p["blocks_w"][c], 64), np.int16) for c in range(nc)]
    tabs = {k: _code_table(*v) for k, v in p["huff"].items()}
    br = _Bits(b, p["scan"])
    pred = [0] * nc
    total = p["mcus_x"] * p["mcus_y"]
    for mcu in range(total):
        if p["restart"] and mcu and mcu % p["restart"] == 0:
            br.restart(0xD0 + ((mcu // p["restart"] - 1) & 7))
            pred = [0] * nc
        my, mx = divmod(mcu, p["mcus_x"])
        for c in range(nc):
            for v in range(p["vs"][c]):
                for h in range(p["hs"][c]):
                    blk = np.zeros(64, np.int64)
                    s = _symbol(br, tabs[(0, p["td"][c])])
                    if s > 15:
                        raise MalformedJpeg("bad DC size")
                    pred[c] += _extend(br.get(s), s)
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = _symbol(br, tabs[(1, p["ta"][c])])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        if k > 63:
                            raise MalformedJpeg("coefficient index past 63")
                        blk[ZIGZAG[k]] = _extend(br.get(s), s)
                        k += 1
                    coef[c][my * p["vs"][c] + v, mx * p["hs"][c] + h] = blk.astype(np.int16)     # wraps like a C cast
    return coef, p["q"].copy()


# ---------------------------------------------------------------------------------------------- dequantisation + inverse DCT
_C = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299, c1847=15137, c1961=16069,
          c2053=16819, c2562=20995, c3072=25172)


def _idct_1d(x, shift):
    """x: (..., 8) int64 -> (..., 8): one pass of libjpeg's jidctint.c, descaled by a rounding right shift"""
    C = _C
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * C["c0541"]
    t2 = z1 - z3 * C["c1847"]
    t3 = z1 + z2 * C["c0765"]
    t0 = (x[..., 0] + x[..., 4]) << 13
    t1 = (x[..., 0] - x[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * C["c1175"]
    o0, o1, o2, o3 = o0 * C["c0298"], o1 * C["c2053"], o2 * C["c3072"], o3 * C["c1501"]
    z1, z2, z3, z4 = -z1 * C["c0899"], -z2 * C["c2562"], -z3 * C["c1961"] + z5, -z4 * C["c0390"] + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    out = np.stack([t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3], -1)
    return (out + (1 << (shift - 1))) >> shift


def range_limit(x):
    """libjpeg's post-IDCT table: index (x & 1023), centred on 128"""
    v = x & 1023
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896))).astype(np.uint8)


def idct_blocks(coef, q):
    """coef (bh, bw, 64) int16, q (64,) -> the padded (bh * 8, bw * 8) uint8 plane"""
    bh, bw, _ = coef.shape
    x = (coef.astype(np.int64) * q.astype(np.int64)).reshape(bh, bw, 8, 8)
    ws = _idct_1d(x.transpose(0, 1, 3, 2), 11).transpose(0, 1, 3, 2)          # columns first
    px = range_limit(_idct_1d(ws, 18))
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


# ---------------------------------------------------------------------------------------------- upsampling + colour
def _h2v1(s):
    s = s.astype(np.int64)
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int64)
    out[:, 0::2] = (3 * s + left + 1) >> 2
    out[:, 1::2] = (3 * s + right + 2) >> 2
    return out


def _h2v2(s):
    s = s.astype(np.int64)
    up = np.concatenate([s[:1], s[:-1]], 0)
    down = np.concatenate([s[1:], s[-1:]], 0)
    out = np.empty((2 * s.shape[0], 2 * s.shape[1]), np.int64)
    for par, nb in ((0, up), (1, down)):
        cs = 3 * s + nb
        left = np.concatenate([cs[:, :1], cs[:, :-1]], 1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        out[par::2, 0::2] = (3 * cs + left + 8) >> 4
        out[par::2, 1::2] = (3 * cs + right + 7) >> 4
    return out


def upsample(plane, H, W, hs, vs):
    """plane: the padded chroma plane; (hs, vs): the luma sampling.  The filter sees the component's own downsampled size only;
    libjpeg replicates instead when that width is 2 or less."""
    if (hs, vs) == (1, 1):
        return plane[:H, :W].astype(np.int64)
    cw, ch = -(-W // hs), -(-H // vs)
    s = plane[:ch, :cw]
    if cw > 2:
        out = _h2v1(s) if vs == 1 else _h2v2(s)
    else:
        out = np.repeat(np.repeat(s, vs, 0), hs, 1).astype(np.int64)
    return out[:H, :W]


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def planes(p, coef, q):
    return [idct_blocks(coef[c], q[p["tq"][c]]) for c in range(p["ncomp"])]


def decode_rgb(data):
    """-> ((H, W, 3) uint8 before the EXIF orientation, orientation), or None for a file that is not covered"""
    p = parse(data)
    if p["status"] != 1:
        return None
    coef, q = entropy_decode(p, data)
    pl = planes(p, coef, q)
    H, W = p["height"], p["width"]
    if p["ncomp"] == 1:
        y = pl[0][:H, :W]
        return np.stack([y, y, y], -1), p["orientation"]
    cb = upsample(pl[1], H, W, p["hs"][0], p["vs"][0])
    cr = upsample(pl[2], H, W, p["hs"][0], p["vs"][0])
    return ycc_to_rgb(pl[0][:H, :W], cb, cr), p["orientation"]


def apply_orientation(a, o):
    """(H, W, C) array -> what Image.transpose gives for EXIF orientation o (detection_utils._apply_exif_orientation)"""
    if o == 2:
        return a[:, ::-1]
    if o == 3:
        return a[::-1, ::-1]
    if o == 4:
        return a[::-1]
    if o == 5:
        return a.transpose(1, 0, 2)
    if o == 6:
        return a.transpose(1, 0, 2)[:, ::-1]
    if o == 7:
        return a.transpose(1, 0, 2)[::-1, ::-1]
    if o == 8:
        return a.transpose(1, 0, 2)[::-1]
    return a


# ---------------------------------------------------------------------------------------------- fixtures
def load_fixtures(golden_dir, groups=("sizes", "content", "streams", "exif")):
    """-> {"group/case": (jpeg bytes as uint8 array, Pillow's (H, W, 3) pixels)}"""
    import os
    out = {}
    for g in groups:
        z = np.load(os.path.join(golden_dir, f"jpeg_{g}.npz"))
        for k in z.files:
            if k.endswith("/jpeg"):
                name = k[:-5]
                out[f"{g}/{name}"] = (z[k], z[name + "/rgb"])
    return out
