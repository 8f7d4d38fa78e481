// Baseline JPEG reader whose pixels equal Pillow's (libjpeg's default decode): the host part parses the markers and undoes the
// Huffman coding, two kernels do the per-pixel work for a whole batch.  See include/soswsod_hip.h for the contract.
//   host    sw_jpeg_probe / sw_jpeg_entropy_decode: plain C++, no HIP call, no globals, nothing read outside bytes[0 .. n)
//   kernel  jpeg_idct_kernel   blocks -> padded u8 component planes (dequantise, jidctint "islow", +128, range limit)
//           jpeg_pixel_kernel  planes -> (3, H, W) pixels (fancy h2v1 / h2v2 upsampling, YCbCr -> RGB, plane order)
// Both kernels run over flat indices of the whole batch (blocks; 4-pixel row pieces) and find their image by bisection over the
// descriptor table, so the launch count and the grid do not depend on how the sizes are mixed.
#include <string.h>

#include "common.h"
#include "soswsod_hip.h"

namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ------------------------------------------------------------------------------------------------ host: markers
struct HuffSpec {
  bool defined;
  uint8_t bits[16];
  uint8_t vals[256];
};

struct Parsed {
  int width, height, ncomp, precision;
  int cid[4], hs[4], vs[4], tq[4], td[4], ta[4];
  int restart, orientation;
  uint16_t q[4][64];
  bool qdef[4];
  HuffSpec huff[2][4];
  long scan;                          // offset of the entropy-coded bytes
};

inline int u16be(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// tag 274 of IFD0 in an APP1 payload of `len` bytes starting at "Exif\0\0"; 0 if absent or unreadable
int exif_orientation(const uint8_t* s, long len) {
  if (len < 14) return 0;
  const uint8_t* t = s + 6;
  const long tl = len - 6;
  bool le;
  if (t[0] == 'I' && t[1] == 'I' && t[2] == 42 && t[3] == 0) le = true;
  else if (t[0] == 'M' && t[1] == 'M' && t[2] == 0 && t[3] == 42) le = false;
  else return 0;
  auto rd = [&](long o, int nb) -> unsigned long {      // caller checks o + nb <= tl
    unsigned long v = 0;
    for (int k = 0; k < nb; ++k) v |= (unsigned long)t[o + (le ? k : nb - 1 - k)] << (8 * k);
    return v;
  };
  const unsigned long ifd = rd(4, 4);
  if (ifd > (unsigned long)tl || (long)ifd + 2 > tl) return 0;
  const long cnt = (long)rd((long)ifd, 2);
  for (long k = 0; k < cnt; ++k) {
    const long e = (long)ifd + 2 + 12 * k;
    if (e + 12 > tl) return 0;
    if (rd(e, 2) == 274) {
      const unsigned long typ = rd(e + 2, 2);
      const unsigned long v = typ == 3 ? rd(e + 8, 2) : typ == 4 ? rd(e + 8, 4) : 0;
      return v >= 1 && v <= 8 ? (int)v : 0;
    }
  }
  return 0;
}

// 1 covered, 0 not covered, < 0 malformed (the codes of the header)
int parse_markers(const uint8_t* b, long n, Parsed& p) {
  if (n < 4 || b[0] != 0xFF || b[1] != 0xD8) return -2;
  memset(&p, 0, sizeof(p));
  p.orientation = 1;
  bool have_sof = false, jfif = false, exif_seen = false;
  int adobe = -1;
  long i = 2;
  for (;;) {
    if (i >= n) return -3;
    if (b[i] != 0xFF) return -4;
    while (i < n && b[i] == 0xFF) ++i;
    if (i >= n) return -3;
    const int m = b[i++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD9 || m == 0xD8 || m == 0) return -4;
    if (i + 2 > n) return -3;
    const long L = u16be(b + i);
    if (L < 2) return -4;
    if (i + L > n) return -3;
    const uint8_t* s = b + i + 2;
    const long sl = L - 2;
    if (m == 0xC0 || m == 0xC1) {
      if (have_sof || sl < 6) return -4;
      const int nc = s[5];
      if (sl != 6 + 3 * nc) return -4;
      p.precision = s[0]; p.height = u16be(s + 1); p.width = u16be(s + 3); p.ncomp = nc;
      if ((p.precision != 8 && p.precision != 12) || p.width == 0 || nc == 0) return -4;
      if (nc > 4) return 0;
      for (int c = 0; c < nc; ++c) {
        p.cid[c] = s[6 + 3 * c]; p.hs[c] = s[7 + 3 * c] >> 4; p.vs[c] = s[7 + 3 * c] & 15; p.tq[c] = s[8 + 3 * c];
        if (p.hs[c] < 1 || p.hs[c] > 4 || p.vs[c] < 1 || p.vs[c] > 4 || p.tq[c] > 3) return -4;
      }
      have_sof = true;
    } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      return 0;                       // progressive, lossless, hierarchical, arithmetic
    } else if (m == 0xC4) {
      long j = 0;
      while (j < sl) {
        if (j + 17 > sl) return -4;
        const int tc = s[j] >> 4, th = s[j] & 15;
        if (tc > 1 || th > 3) return -4;
        int cnt = 0, code = 0;
        for (int l = 0; l < 16; ++l) {
          cnt += s[j + 1 + l];
          code += s[j + 1 + l];
          if (code > (1 << (l + 1))) return -4;
          code <<= 1;
        }
        if (cnt > 256 || j + 17 + cnt > sl) return -4;
        HuffSpec& h = p.huff[tc][th];
        h.defined = true;
        memcpy(h.bits, s + j + 1, 16);
        memset(h.vals, 0, sizeof(h.vals));
        memcpy(h.vals, s + j + 17, cnt);
        j += 17 + cnt;
      }
    } else if (m == 0xDB) {
      long j = 0;
      while (j < sl) {
        const int pq = s[j] >> 4, tq = s[j] & 15;
        const int sz = pq ? 128 : 64;
        if (pq > 1 || tq > 3 || j + 1 + sz > sl) return -4;
        for (int k = 0; k < 64; ++k) p.q[tq][kZigzag[k]] = (uint16_t)(pq ? u16be(s + j + 1 + 2 * k) : s[j + 1 + k]);
        p.qdef[tq] = true;
        j += 1 + sz;
      }
    } else if (m == 0xDD) {
      if (sl != 2) return -4;
      p.restart = u16be(s);
    } else if (m == 0xE0 && sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) {
      jfif = true;
    } else if (m == 0xE1 && sl >= 6 && memcmp(s, "Exif\0\0", 6) == 0 && !exif_seen) {
      exif_seen = true;
      const int o = exif_orientation(s, sl);
      p.orientation = o ? o : 1;
    } else if (m == 0xEE && sl >= 12 && memcmp(s, "Adobe", 5) == 0) {
      adobe = s[11];
    } else if (m == 0xDA) {
      if (!have_sof) return -5;
      if (sl < 1 || sl != 4 + 2 * s[0]) return -4;
      const int nc = p.ncomp;
      if (p.precision != 8 || p.height == 0 || (nc != 1 && nc != 3) || s[0] != nc) return 0;
      for (int c = 0; c < nc; ++c) {
        if (s[1 + 2 * c] != p.cid[c]) return -4;
        p.td[c] = s[2 + 2 * c] >> 4; p.ta[c] = s[2 + 2 * c] & 15;
      }
      if (s[1 + 2 * nc] != 0 || s[2 + 2 * nc] != 63 || s[3 + 2 * nc] != 0) return -4;
      if (nc == 1) {
        if (p.hs[0] != 1 || p.vs[0] != 1) return 0;
      } else {
        const bool luma_ok = (p.hs[0] == 1 && p.vs[0] == 1) || (p.hs[0] == 2 && p.vs[0] == 1) || (p.hs[0] == 2 && p.vs[0] == 2);
        if (!luma_ok || p.hs[1] != 1 || p.vs[1] != 1 || p.hs[2] != 1 || p.vs[2] != 1) return 0;
        if (adobe >= 0) {
          if (adobe != 1) return 0;
        } else if (!jfif && p.cid[0] == 'R' && p.cid[1] == 'G' && p.cid[2] == 'B') {
          return 0;
        }
      }
      for (int c = 0; c < nc; ++c) {
        if (!p.qdef[p.tq[c]]) return -5;
        if (p.td[c] > 3 || p.ta[c] > 3 || !p.huff[0][p.td[c]].defined || !p.huff[1][p.ta[c]].defined) return -5;
      }
      p.scan = i + L;
      return 1;
    }
    i += L;
  }
}

void fill_info(const Parsed& p, sw_jpeg_info* info) {
  memset(info, 0, sizeof(*info));
  info->width = p.width; info->height = p.height; info->ncomp = p.ncomp;
  info->restart_interval = p.restart; info->orientation = p.orientation;
  info->mcus_x = (p.width + 8 * p.hs[0] - 1) / (8 * p.hs[0]);
  info->mcus_y = (p.height + 8 * p.vs[0] - 1) / (8 * p.vs[0]);
  int64_t blocks = 0;
  for (int c = 0; c < p.ncomp; ++c) {
    info->hsamp[c] = p.hs[c]; info->vsamp[c] = p.vs[c]; info->qtable[c] = p.tq[c];
    info->blocks_w[c] = info->mcus_x * p.hs[c];
    info->blocks_h[c] = info->mcus_y * p.vs[c];
    blocks += (int64_t)info->blocks_w[c] * info->blocks_h[c];
  }
  info->coef_bytes = 128 * blocks;
}

// ------------------------------------------------------------------------------------------------ host: Huffman
constexpr int kLutBits = 10;

struct HuffTable {
  uint16_t lut[1 << kLutBits];        // (length << 8) | symbol for codes of <= kLutBits bits, else 0
  int32_t maxcode[18];                // largest code of each length, -1 if none; [17] ends the search
  int32_t valoff[17];                 // vals index of a length's first code minus that code
  const uint8_t* vals;
};

void build_table(const HuffSpec& h, HuffTable& t) {
  memset(t.lut, 0, sizeof(t.lut));
  t.vals = h.vals;
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = h.bits[l - 1];
    t.valoff[l] = k - code;
    if (l <= kLutBits) {
      for (int c = 0; c < cnt; ++c) {
        const int first = (code + c) << (kLutBits - l);
        for (int f = 0; f < (1 << (kLutBits - l)); ++f) t.lut[first + f] = (uint16_t)((l << 8) | h.vals[k + c]);
      }
    }
    code += cnt;
    k += cnt;
    t.maxcode[l] = cnt ? code - 1 : -1;
    code <<= 1;
  }
  t.maxcode[17] = 0x7FFFFFFF;
}

// MSB-first bit reader over the entropy-coded bytes: FF 00 is a data byte FF, FF FF.. are fill bytes, any other FF xx is a marker.
// Behind a marker or the end of the buffer it supplies zero bits and counts them in `fake`; they sit at the tail of the
// buffer, so `cnt < fake` says that bits which do not exist were consumed.
struct BitReader {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t buf;
  int cnt, fake, marker;              // marker: 0 none yet, 0x100 the buffer's end, else the marker's code (p is behind it)

  inline void fill() {
    while (cnt <= 56) {
      unsigned byte = 0;
      if (!marker && p < end) {
        byte = *p++;
        if (byte == 0xFF) {
          while (p < end && *p == 0xFF) ++p;
          if (p >= end) { marker = 0x100; byte = 0; fake += 8; }
          else if (*p == 0) { ++p; }
          else { marker = *p++; byte = 0; fake += 8; }
        }
      } else {
        if (!marker) marker = 0x100;
        fake += 8;
      }
      buf |= (uint64_t)byte << (56 - cnt);
      cnt += 8;
    }
  }
  inline unsigned peek(int k) const { return (unsigned)(buf >> (64 - k)); }      // 1 <= k <= 32
  inline void skip(int k) { buf <<= k; cnt -= k; }
};

// one symbol; -1: no code of up to 16 bits matches.  Needs >= 16 bits in the buffer.
inline int decode_symbol(BitReader& br, const HuffTable& t) {
  const unsigned e = t.lut[br.peek(kLutBits)];
  if (e) { br.skip(e >> 8); return e & 255; }
  const int top = (int)br.peek(16);
  int l = kLutBits + 1;
  while (l <= 16 && (top >> (16 - l)) > t.maxcode[l]) ++l;
  if (l > 16) return -1;
  const int idx = t.valoff[l] + (top >> (16 - l));
  if (idx < 0 || idx > 255) return -1;
  br.skip(l);
  return t.vals[idx];
}

inline int receive_extend(BitReader& br, int s) {       // 1 <= s <= 16
  const int v = (int)br.peek(s);
  br.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

int entropy_decode(const uint8_t* b, long n, const Parsed& p, const sw_jpeg_info& info, int16_t* coef) {
  HuffTable dc[3], ac[3];
  int16_t* base[3];
  int16_t* q = coef;
  for (int c = 0; c < p.ncomp; ++c) {
    build_table(p.huff[0][p.td[c]], dc[c]);
    build_table(p.huff[1][p.ta[c]], ac[c]);
    base[c] = q;
    q += (long)info.blocks_w[c] * info.blocks_h[c] * 64;
  }
  BitReader br = {b + p.scan, b + n, 0, 0, 0, 0};
  int pred[3] = {0, 0, 0};
  const long total = (long)info.mcus_x * info.mcus_y;
  int mx = 0, my = 0;
  long until_restart = p.restart ? p.restart : -1;
  int next_rst = 0;
  for (long mcu = 0; mcu < total; ++mcu) {
    if (until_restart == 0) {
      br.fill();
      if (br.cnt - br.fake >= 8) return -8;                          // whole data bytes in front of the marker
      if (br.marker != 0xD0 + next_rst) return br.marker == 0x100 ? -6 : -8;
      next_rst = (next_rst + 1) & 7;
      br.buf = 0; br.cnt = 0; br.fake = 0; br.marker = 0;
      pred[0] = pred[1] = pred[2] = 0;
      until_restart = p.restart;
    }
    for (int c = 0; c < p.ncomp; ++c) {
      for (int v = 0; v < p.vs[c]; ++v) {
        for (int h = 0; h < p.hs[c]; ++h) {
          int16_t* blk = base[c] + ((long)(my * p.vs[c] + v) * info.blocks_w[c] + (mx * p.hs[c] + h)) * 64;
          br.fill();
          int s = decode_symbol(br, dc[c]);
          if (s < 0 || s > 15) return br.cnt < br.fake ? -6 : -7;
          if (s) pred[c] += receive_extend(br, s);
          blk[0] = (int16_t)pred[c];
          for (int k = 1; k < 64;) {
            br.fill();
            const int rs = decode_symbol(br, ac[c]);
            if (rs < 0) return br.cnt < br.fake ? -6 : -7;
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
              if (r != 15) break;
              k += 16;
              continue;
            }
            k += r;
            if (k > 63) return br.cnt < br.fake ? -6 : -7;
            blk[kZigzag[k]] = (int16_t)receive_extend(br, s);
            ++k;
          }
          if (br.cnt < br.fake) return -6;
        }
      }
    }
    if (++mx == info.mcus_x) { mx = 0; ++my; }
    if (until_restart > 0) --until_restart;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ device
__device__ __forceinline__ int find_by_block(const sw_jpeg_desc* d, int n, int key) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].block_start <= key) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ int find_by_quad(const sw_jpeg_desc* d, int n, int key) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].quad_start <= key) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// One pass of libjpeg's jidctint.c over 8 values, descaled by a rounding arithmetic right shift.  The sums are formed in unsigned
// words (wrap instead of overflow on coefficients no encoder produces); identical to the signed arithmetic wherever that is defined.
__device__ __forceinline__ void idct8(const int* x, int shift, int* o) {
  typedef unsigned int U;
  const U x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3], x4 = x[4], x5 = x[5], x6 = x[6], x7 = x[7];
  U z1 = (x2 + x6) * 4433u;
  const U t2 = z1 - x6 * 15137u;
  const U t3 = z1 + x2 * 6270u;
  const U t0 = (x0 + x4) << 13;
  const U t1 = (x0 - x4) << 13;
  const U t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  U o0 = x7, o1 = x5, o2 = x3, o3 = x1;
  z1 = o0 + o3;
  U z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const U z5 = (z3 + z4) * 9633u;
  o0 *= 2446u; o1 *= 16819u; o2 *= 25172u; o3 *= 12299u;
  z1 = 0u - z1 * 7373u; z2 = 0u - z2 * 20995u; z3 = z5 - z3 * 16069u; z4 = z5 - z4 * 3196u;
  o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
  const U r = 1u << (shift - 1);
  o[0] = (int)(t10 + o3 + r) >> shift; o[7] = (int)(t10 - o3 + r) >> shift;
  o[1] = (int)(t11 + o2 + r) >> shift; o[6] = (int)(t11 - o2 + r) >> shift;
  o[2] = (int)(t12 + o1 + r) >> shift; o[5] = (int)(t12 - o1 + r) >> shift;
  o[3] = (int)(t13 + o0 + r) >> shift; o[4] = (int)(t13 - o0 + r) >> shift;
}

// libjpeg's post-IDCT range-limit table, indexed by (x & 1023), centred on 128
__device__ __forceinline__ unsigned range_limit(int x) {
  const int v = x & 1023;
  return v < 128 ? v + 128 : v < 512 ? 255 : v < 896 ? 0 : v - 896;
}

constexpr int kBlocksPerGroup = 32;     // 256 threads: 8 per block (one row, then one column, then one row of it)
constexpr int kWsStride = 72;           // ints per block in LDS: rows 9 apart, blocks 72 apart -> both passes conflict-free

__global__ __launch_bounds__(256) void jpeg_idct_kernel(int n, const sw_jpeg_desc* __restrict__ descs, int total_blocks,
                                                        const int16_t* __restrict__ coef, const uint16_t* __restrict__ qtables,
                                                        uint8_t* __restrict__ workspace) {
  __shared__ int ws[kBlocksPerGroup * kWsStride];
  const int lb = threadIdx.x >> 3, j = threadIdx.x & 7;
  const int g = blockIdx.x * kBlocksPerGroup + lb;
  const bool live = g < total_blocks;
  int* w = ws + lb * kWsStride;
  uint8_t* dst = nullptr;
  if (live) {
    const sw_jpeg_desc& D = descs[find_by_block(descs, n, g)];
    int k = g - D.block_start, c = 0;
    int64_t plane = D.plane_off;
    while (c + 1 < D.ncomp && k >= D.blocks_w[c] * D.blocks_h[c]) {
      k -= D.blocks_w[c] * D.blocks_h[c];
      plane += 64L * D.blocks_w[c] * D.blocks_h[c];
      ++c;
    }
    const int bw = D.blocks_w[c], by = k / bw, bx = k - by * bw;
    dst = workspace + plane + ((int64_t)(by * 8 + j) * bw + bx) * 8;
    const s16x8 cv = *(const s16x8*)(coef + D.coef_off + (int64_t)(g - D.block_start) * 64 + j * 8);
    const s16x8 qv = *(const s16x8*)(qtables + D.qtab_off + D.qtable[c] * 64 + j * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) w[j * 9 + i] = (int)cv[i] * (int)(unsigned short)qv[i];
  }
  __syncthreads();
  int x[8], o[8];
  if (live) {
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] = w[r * 9 + j];
    idct8(x, 11, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r * 9 + j] = o[r];
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = w[j * 9 + i];
    idct8(x, 18, o);
    u32x2 px;
    px[0] = range_limit(o[0]) | range_limit(o[1]) << 8 | range_limit(o[2]) << 16 | range_limit(o[3]) << 24;
    px[1] = range_limit(o[4]) | range_limit(o[5]) << 8 | range_limit(o[6]) << 16 | range_limit(o[7]) << 24;
    *(u32x2*)dst = px;
  }
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// one upsampled chroma sample at (y, x) of the image.  s: the padded plane, `stride` bytes per row; cw, ch: the component's own
// downsampled size, which is where the filter's edges are.  libjpeg replicates instead of filtering when cw <= 2.
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ s, int stride, int cw, int ch, int hs, int vs, int y, int x) {
  if (hs == 1) return s[(long)y * stride + x];
  const int i = x >> 1;
  if (cw <= 2) return s[(long)(vs == 2 ? y >> 1 : y) * stride + i];
  const int in = (x & 1) ? min(i + 1, cw - 1) : max(i - 1, 0);
  if (vs == 1) {
    const uint8_t* row = s + (long)y * stride;
    return (3 * row[i] + row[in] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int r = y >> 1;
  const int rn = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
  const uint8_t* r0 = s + (long)r * stride;
  const uint8_t* r1 = s + (long)rn * stride;
  const int cs = 3 * r0[i] + r1[i], csn = 3 * r0[in] + r1[in];
  return (3 * cs + csn + ((x & 1) ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_pixel_kernel(int n, const sw_jpeg_desc* __restrict__ descs, int total_quads,
                                                         const uint8_t* __restrict__ workspace) {
  const int qd = blockIdx.x * 256 + threadIdx.x;
  if (qd >= total_quads) return;
  const sw_jpeg_desc& D = descs[find_by_quad(descs, n, qd)];
  const int W = D.width, H = D.height;
  const int qpr = (W + 3) >> 2;
  const int lq = qd - D.quad_start;
  const int y = lq / qpr, x0 = (lq - y * qpr) * 4;
  const int ystride = D.blocks_w[0] * 8;
  const uint8_t* yp = workspace + D.plane_off;
  const unsigned yy = *(const unsigned*)(yp + (long)y * ystride + x0);          // x0 + 3 lies inside the padded row
  unsigned pr = 0, pg = 0, pb = 0;
  if (D.ncomp == 1) {
    pr = pg = pb = yy;
  } else {
    const int hs = D.hsamp, vs = D.vsamp;
    const int cstride = D.blocks_w[1] * 8;
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
    const uint8_t* cbp = yp + 64L * D.blocks_w[0] * D.blocks_h[0];
    const uint8_t* crp = cbp + 64L * D.blocks_w[1] * D.blocks_h[1];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = min(x0 + k, W - 1);                                         // past the row's end: recomputed, never stored
      const int Y = (yy >> (8 * k)) & 255;
      const int cb = chroma_at(cbp, cstride, cw, ch, hs, vs, y, x) - 128;
      const int cr = chroma_at(crp, cstride, cw, ch, hs, vs, y, x) - 128;
      pr |= (unsigned)clamp255(Y + ((91881 * cr + 32768) >> 16)) << (8 * k);
      pg |= (unsigned)clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)) << (8 * k);
      pb |= (unsigned)clamp255(Y + ((116130 * cb + 32768) >> 16)) << (8 * k);
    }
  }
  const long plane = (long)H * W;
  uint8_t* o0 = D.out + (long)y * W + x0;
  const unsigned first = D.bgr ? pb : pr, third = D.bgr ? pr : pb;
  if ((W & 3) == 0 && (((uintptr_t)D.out) & 3) == 0) {
    *(unsigned*)o0 = first;
    *(unsigned*)(o0 + plane) = pg;
    *(unsigned*)(o0 + 2 * plane) = third;
  } else {
    for (int k = 0; k < 4 && x0 + k < W; ++k) {
      o0[k] = (uint8_t)(first >> (8 * k));
      o0[plane + k] = (uint8_t)(pg >> (8 * k));
      o0[2 * plane + k] = (uint8_t)(third >> (8 * k));
    }
  }
}

bool info_ok(const sw_jpeg_info& f) {
  if (f.width <= 0 || f.height <= 0 || f.width > 65535 || f.height > 65535 || (f.ncomp != 1 && f.ncomp != 3)) return false;
  const int hs = f.hsamp[0], vs = f.vsamp[0];
  if (f.ncomp == 1 ? (hs != 1 || vs != 1) : !((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
  if (f.mcus_x != (f.width + 8 * hs - 1) / (8 * hs) || f.mcus_y != (f.height + 8 * vs - 1) / (8 * vs)) return false;
  int64_t blocks = 0;
  for (int c = 0; c < f.ncomp; ++c) {
    if (c > 0 && (f.hsamp[c] != 1 || f.vsamp[c] != 1)) return false;
    if (f.qtable[c] < 0 || f.qtable[c] > 3) return false;
    if (f.blocks_w[c] != f.mcus_x * f.hsamp[c] || f.blocks_h[c] != f.mcus_y * f.vsamp[c]) return false;
    blocks += (int64_t)f.blocks_w[c] * f.blocks_h[c];
  }
  return f.coef_bytes == 128 * blocks;
}

}  // namespace

extern "C" int sw_jpeg_probe(const uint8_t* bytes, long n, sw_jpeg_info* info) {
  if (!bytes || !info || n < 0) return -1;
  Parsed p;
  const int rc = parse_markers(bytes, n, p);
  if (rc == 1) fill_info(p, info);
  return rc;
}

extern "C" int sw_jpeg_entropy_decode(const uint8_t* bytes, long n, const sw_jpeg_info* info, int16_t* coef, uint16_t* qtables) {
  if (!bytes || !info || !coef || !qtables || n < 0) return -1;
  Parsed p;
  const int rc = parse_markers(bytes, n, p);
  if (rc < 0) return rc;
  if (rc == 0) return -9;
  sw_jpeg_info now;
  fill_info(p, &now);
  if (memcmp(&now, info, sizeof(now)) != 0) return -9;
  memset(coef, 0, (size_t)now.coef_bytes);
  memcpy(qtables, p.q, sizeof(p.q));
  return entropy_decode(bytes, n, p, now, coef);
}

extern "C" const char* sw_jpeg_strerror(int code) {
  switch (code) {
    case 1: return "covered";
    case 0: return "not covered by the device decoder";
    case -1: return "bad argument";
    case -2: return "no SOI marker: not a JPEG stream";
    case -3: return "the marker segments end early";
    case -4: return "malformed marker segment";
    case -5: return "frame, quantisation table or Huffman table missing";
    case -6: return "the entropy-coded data ends early";
    case -7: return "invalid Huffman code or coefficient index";
    case -8: return "restart marker missing or out of sequence";
    case -9: return "the info does not describe this stream";
    default: return "unknown code";
  }
}

extern "C" long sw_jpeg_workspace_bytes(int n_images, const sw_jpeg_info* infos) {
  if (n_images < 0 || (n_images > 0 && !infos)) return -1;
  long total = 0;
  for (int i = 0; i < n_images; ++i) {
    if (!info_ok(infos[i])) return -1;
    total += infos[i].coef_bytes / 2;
  }
  return total;
}

extern "C" int sw_jpeg_describe_batch(int n_images, const sw_jpeg_info* infos, void* const* outs, int bgr, sw_jpeg_desc* descs,
                                      long* total_blocks, long* total_quads) {
  if (n_images < 0 || !total_blocks || !total_quads || (n_images > 0 && (!infos || !outs || !descs))) return -1;
  long blocks = 0, quads = 0;
  for (int i = 0; i < n_images; ++i) {
    const sw_jpeg_info& f = infos[i];
    if (!info_ok(f) || !outs[i]) return -1;
    sw_jpeg_desc& d = descs[i];
    memset(&d, 0, sizeof(d));
    d.out = (uint8_t*)outs[i];
    d.coef_off = blocks * 64; d.qtab_off = 256L * i; d.plane_off = blocks * 64;
    d.block_start = (int32_t)blocks; d.quad_start = (int32_t)quads;
    d.width = f.width; d.height = f.height; d.ncomp = f.ncomp; d.hsamp = f.hsamp[0]; d.vsamp = f.vsamp[0]; d.bgr = bgr ? 1 : 0;
    for (int c = 0; c < f.ncomp; ++c) { d.blocks_w[c] = f.blocks_w[c]; d.blocks_h[c] = f.blocks_h[c]; d.qtable[c] = f.qtable[c]; }
    blocks += f.coef_bytes / 128;
    quads += (long)f.height * ((f.width + 3) / 4);
    if (blocks >= (1L << 31) - 64 || quads >= (1L << 31) - 256) return -6;
  }
  *total_blocks = blocks; *total_quads = quads;
  return 0;
}

extern "C" int sw_jpeg_decode_batch(int n_images, const sw_jpeg_desc* descs, long total_blocks, long total_quads, const int16_t* coef,
                                    const uint16_t* qtables, uint8_t* workspace, hipStream_t stream) {
  SW_ENTER();
  if (n_images < 0 || total_blocks < 0 || total_quads < 0) return -1;
  if (n_images == 0) return 0;
  if (!descs || !coef || !qtables || !workspace || total_blocks < n_images || total_quads < n_images) return -1;
  if (total_blocks >= (1L << 31) - 64 || total_quads >= (1L << 31) - 256) return -6;
  if (((uintptr_t)coef & 15) || ((uintptr_t)qtables & 15) || ((uintptr_t)workspace & 255) || ((uintptr_t)descs & 7)) return -4;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((total_blocks + kBlocksPerGroup - 1) / kBlocksPerGroup)), dim3(256), 0, stream,
                     n_images, descs, (int)total_blocks, coef, qtables, workspace);
  hipLaunchKernelGGL(jpeg_pixel_kernel, dim3((unsigned)((total_quads + 255) / 256)), dim3(256), 0, stream, n_images, descs,
                     (int)total_quads, (const uint8_t*)workspace);
  SW_CHECK_LAUNCH();
  return 0;
}
