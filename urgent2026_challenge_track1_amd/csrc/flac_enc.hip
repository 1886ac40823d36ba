// FLAC stream ENCODER on the device (mono, 16 bit): the writer of the offline simulator (simulation/simulate_data_from_param.py:
// 572-586 -> soundfile.write, '--out_format flac' is the reference's default) once the DSP runs batched on the GPU.
// Written from the published format specification (xiph.org FLAC format): fixed-blocksize frames, one workgroup per frame,
// CONSTANT / VERBATIM / FIXED (order 0-4) subframes, partitioned Rice residuals with the 4-bit parameter (k <= 14, no escape
// partitions), CRC-8 / CRC-16.  The host prepends 'fLaC' + STREAMINFO (flac.py).
//
// One frame, one workgroup of 256 threads:
//   1. the frame's samples go to LDS; a frame of equal samples is a CONSTANT subframe;
//   2. for every FIXED order a wave takes 64 consecutive residuals at a time (lane = sample) and counts, per bit plane b of the
//      zigzag value u, the lanes that have it set (ballot + popcount).  sum_i (u_i >> k) = sum_{b >= k} count_b << (b - k), so lane k
//      of the wave gets the EXACT unary cost of its 64 residuals under Rice parameter k without a single reduction over lanes;
//   3. a prefix over the 64-sample chunks gives the exact cost of every partition of every partition order under every k; the
//      cheapest k per partition, the cheapest partition order per FIXED order and the cheapest order are kept (ties: the lower one);
//   4. code lengths are scanned over the workgroup and every thread ORs its codes (MSB first) into a zeroed LDS image of the frame;
//   5. CRC-16 of the image: every thread takes a run of bytes, the partial CRCs are combined in a tree (the CRC is linear:
//      crc(A || B) = crc(A) x^(8 |B|) + crc(B) over GF(2) mod the generator), and the image is flushed with coalesced dword stores.
// Every choice is an integer minimum in a fixed order: the bytes of a frame depend on its samples, length, rate and number only.
#include <vector>

#include "urse_common.h"

namespace urse {

constexpr int FE_THREADS = 256;
constexpr int FE_MAXBS = 4096;
constexpr int FE_PLANES = 22;                       // zigzag of a 21-bit order-4 residual of 16-bit samples
constexpr int FE_MAXK = 14;                         // 4-bit Rice parameter, 15 = escape (not used)
constexpr int FE_MAXCH = FE_MAXBS / 64;             // 64-sample chunks per frame
constexpr int FE_SLOT_EXTRA = 32;                   // header (<= 15 bytes) + subframe byte + CRC-16, rounded so that slots stay 16-byte aligned
constexpr int FE_OUT_WORDS = (2 * FE_MAXBS + FE_SLOT_EXTRA) / 4;
constexpr unsigned FE_CLAMP = 1u << 20;             // a chunk cost above this loses to k = 14 (64 * (15 + 128) bits) anyway

struct FlacFrameDesc {
  int64_t off;          // first sample of the frame in the concatenated PCM
  int32_t n_rate;       // samples in the frame | sample-rate code << 16
  int32_t fno;          // frame number inside its file
};

__device__ __forceinline__ int fe_uidx(int i) { return i + (i >> 4); }      // 16 consecutive values per thread: pitch 17, no bank conflict

// ORs the low nb (<= 16) bits of val into the big-endian bit image W at bit position pos
__device__ __forceinline__ void fe_put(unsigned* W, unsigned val, int nb, int pos) {
  const int w = pos >> 5, sh = pos & 31;
  const unsigned long long v = (unsigned long long)(val & ((1u << nb) - 1u)) << (64 - nb - sh);
  const unsigned hi = (unsigned)(v >> 32), lo = (unsigned)v;
  if (hi && w < FE_OUT_WORDS) atomicOr(&W[w], hi);
  if (lo && w + 1 < FE_OUT_WORDS) atomicOr(&W[w + 1], lo);
}
__device__ __forceinline__ unsigned fe_byte(const unsigned* W, int j) { return (W[j >> 2] >> (24 - 8 * (j & 3))) & 0xffu; }

__device__ __forceinline__ int fe_utf8_len(unsigned v) {
  return v < 0x80u ? 1 : v < 0x800u ? 2 : v < 0x10000u ? 3 : v < 0x200000u ? 4 : v < 0x4000000u ? 5 : 6;
}

// a * b over GF(2) modulo x^16 + x^15 + x^2 + 1
__device__ __forceinline__ unsigned fe_mulmod16(unsigned a, unsigned b) {
  unsigned r = 0;
#pragma unroll
  for (int i = 15; i >= 0; --i) {
    r = ((r << 1) ^ ((r & 0x8000u) ? 0x8005u : 0u)) & 0xffffu;
    if ((b >> i) & 1u) r ^= a;
  }
  return r;
}

// Residuals of one FIXED order -> E[c][k] = sum over chunk c of (u >> k), then (in place) the exclusive prefix over chunks, E[nch] = total.
__device__ void fe_analyse(const short* S, unsigned* U, unsigned (*E)[16], int n, int order, bool store) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = (n + 63) >> 6;
  for (int c = wave; c < nch; c += FE_THREADS / 64) {
    const int i = c * 64 + lane;
    unsigned u = 0;
    if (i < n && i >= order) {
      int r = S[i];
      if (order == 1) r -= S[i - 1];
      else if (order == 2) r += -2 * S[i - 1] + S[i - 2];
      else if (order == 3) r += -3 * S[i - 1] + 3 * S[i - 2] - S[i - 3];
      else if (order == 4) r += -4 * S[i - 1] + 6 * S[i - 2] - 4 * S[i - 3] + S[i - 4];
      u = ((unsigned)r << 1) ^ (unsigned)(r >> 31);
    }
    if (store && i < n) U[fe_uidx(i)] = u;
    unsigned e = 0;
#pragma unroll
    for (int b = 0; b < FE_PLANES; ++b) {
      const unsigned cnt = (unsigned)__popcll(__ballot((u >> b) & 1u));
      e += b >= lane ? cnt << ((b - lane) & 31) : 0u;
    }
    if (lane <= FE_MAXK) E[c][lane] = e < FE_CLAMP ? e : FE_CLAMP;
  }
  __syncthreads();
  if (threadIdx.x <= FE_MAXK) {
    unsigned run = 0;
    for (int c = 0; c < nch; ++c) {
      const unsigned v = E[c][threadIdx.x];
      E[c][threadIdx.x] = run;
      run += v;
    }
    E[nch][threadIdx.x] = run;
  }
  __syncthreads();
}

// Every partition of every partition order 0 .. pmax: item (1 << p) - 1 + j = partition j of order p -> its cheapest k and bits
// (parameter included); LV[p] = the bits of the whole residual under partition order p.
__device__ void fe_partitions(unsigned (*E)[16], int* PB, int* PK, int* LV, int n, int order, int pmax) {
  const int t = threadIdx.x, nch = (n + 63) >> 6;
  if (t < (2 << pmax) - 1) {
    const int p = 31 - __clz(t + 1), j = t + 1 - (1 << p);
    const int c0 = p ? j * (nch >> p) : 0, c1 = p ? (j + 1) * (nch >> p) : nch;
    const int cnt = (n >> p) - (j == 0 ? order : 0);
    int best = 0x7fffffff, bk = 0;
    for (int k = 0; k <= FE_MAXK; ++k) {
      const int bits = cnt * (k + 1) + (int)(E[c1][k] - E[c0][k]);
      if (bits < best) { best = bits; bk = k; }
    }
    PB[t] = best + 4;
    PK[t] = bk;
  }
  __syncthreads();
  if (t <= pmax) {
    int sum = 0;
    for (int j = 0; j < (1 << t); ++j) sum += PB[(1 << t) - 1 + j];
    LV[t] = sum;
  }
  __syncthreads();
}

__global__ __launch_bounds__(FE_THREADS) void flac_encode_frames_kernel(const int16_t* __restrict__ pcm,
                                                                        const FlacFrameDesc* __restrict__ desc,
                                                                        unsigned char* __restrict__ slots, int32_t* __restrict__ frame_bytes,
                                                                        int bs, int slot_stride) {
  __shared__ short S[FE_MAXBS];
  __shared__ unsigned U[FE_MAXBS + FE_MAXBS / 16];
  __shared__ unsigned W[FE_OUT_WORDS];
  __shared__ unsigned E[FE_MAXCH + 1][16];
  __shared__ int PB[2 * FE_MAXCH], PK[2 * FE_MAXCH], LV[8], SC[FE_THREADS / 64];
  __shared__ unsigned CR[FE_THREADS];
  __shared__ int best_bits, best_o, best_p;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t f = blockIdx.x;
  const FlacFrameDesc d = desc[f];
  const int n = d.n_rate & 0xffff, rate_code = d.n_rate >> 16;
  const unsigned fno = (unsigned)d.fno;
  const int16_t* x = pcm + d.off;

  for (int i = t; i < n; i += FE_THREADS) S[i] = x[i];
  const int words = (2 * bs + FE_SLOT_EXTRA) / 4;
  for (int i = t; i < words; i += FE_THREADS) W[i] = 0;
  if (t == 0) { best_bits = 16 * n; best_o = -1; best_p = 0; }      // -1: VERBATIM
  __syncthreads();
  int differs = 0;
  for (int i = t; i < n; i += FE_THREADS) differs |= S[i] != S[0];
  const bool constant = !__syncthreads_or(differs);

  // ---- the cheapest subframe ----
  const int pmax = n == bs ? 31 - __clz(bs >> 6) : 0;      // partitions are whole 64-sample chunks; a short last block has one partition
  if (!constant) {
    const int omax = n - 1 < 4 ? n - 1 : 4;
    for (int o = 0; o <= omax; ++o) {
      fe_analyse(S, U, E, n, o, false);
      fe_partitions(E, PB, PK, LV, n, o, pmax);
      if (t == 0) {
        for (int p = 0; p <= pmax; ++p) {
          const int bits = 16 * o + 6 + LV[p];
          if (bits < best_bits) { best_bits = bits; best_o = o; best_p = p; }
        }
      }
      __syncthreads();
    }
  }
  const int o = best_o, p = best_p;

  // ---- frame header ----
  const int hlen = 4 + fe_utf8_len(fno) + (n == bs ? 0 : n <= 256 ? 1 : 2) + 1;
  if (t == 0) {
    unsigned char hb[16];
    int h = 0;
    hb[h++] = 0xff; hb[h++] = 0xf8;                                   // sync, fixed block size
    const int bs_code = n == bs ? 8 + (31 - __clz(bs >> 8)) : n <= 256 ? 6 : 7;
    hb[h++] = (unsigned char)(bs_code << 4 | rate_code);
    hb[h++] = 0x08;                                                   // mono, 16 bit
    const int ul = fe_utf8_len(fno);
    if (ul == 1) hb[h++] = (unsigned char)fno;
    else {
      hb[h++] = (unsigned char)((0xff00u >> ul) & 0xffu) | (unsigned char)(fno >> (6 * (ul - 1)));
      for (int i = ul - 2; i >= 0; --i) hb[h++] = (unsigned char)(0x80u | ((fno >> (6 * i)) & 0x3fu));
    }
    if (bs_code == 6) hb[h++] = (unsigned char)(n - 1);
    else if (bs_code == 7) { hb[h++] = (unsigned char)((n - 1) >> 8); hb[h++] = (unsigned char)((n - 1) & 0xff); }
    unsigned c8 = 0;
    for (int i = 0; i < h; ++i) {
      c8 ^= hb[i];
      for (int b = 0; b < 8; ++b) c8 = (c8 & 0x80u) ? ((c8 << 1) ^ 0x07u) & 0xffu : (c8 << 1) & 0xffu;
    }
    hb[h++] = (unsigned char)c8;
    for (int i = 0; i < h; ++i) fe_put(W, hb[i], 8, 8 * i);
    // subframe header: 0 | type (6) | no wasted bits
    const unsigned type = constant ? 0u : o < 0 ? 1u : 8u + (unsigned)o;
    fe_put(W, type << 1, 8, 8 * h);
  }
  const int base = 8 * (hlen + 1);
  int total_bits;
  if (constant) {
    if (t == 0) fe_put(W, (unsigned)S[0], 16, base);
    total_bits = base + 16;
  } else if (o < 0) {
    for (int i = t; i < n; i += FE_THREADS) fe_put(W, (unsigned)S[i], 16, base + 16 * i);
    total_bits = base + 16 * n;
  } else {
    fe_analyse(S, U, E, n, o, true);
    fe_partitions(E, PB, PK, LV, n, o, pmax);
    if (t < o) fe_put(W, (unsigned)S[t], 16, base + 16 * t);          // warm-up samples
    if (t == 0) fe_put(W, (unsigned)p, 6, base + 16 * o);             // Rice method 0, partition order
    const int rbase = base + 16 * o + 6;
    const int cpt = bs / FE_THREADS, i0 = t * cpt;
    const int lm = 31 - __clz(bs) - p;                                 // log2 of the partition length (p > 0 only when n == bs)
    int mine = 0;
    for (int i = i0; i < i0 + cpt && i < n; ++i) {
      if (i < o) continue;
      const int j = p ? i >> lm : 0;
      const int k = PK[(1 << p) - 1 + j];
      const bool first = i == (j ? j << lm : o);
      mine += (int)(U[fe_uidx(i)] >> k) + 1 + k + (first ? 4 : 0);
    }
    int incl = mine;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const int v = __shfl_up(incl, s, 64);
      if (lane >= s) incl += v;
    }
    if (lane == 63) SC[wave] = incl;
    __syncthreads();
    int pos = rbase + incl - mine;
    for (int w = 0; w < wave; ++w) pos += SC[w];
    total_bits = rbase;
    for (int w = 0; w < FE_THREADS / 64; ++w) total_bits += SC[w];
    for (int i = i0; i < i0 + cpt && i < n; ++i) {
      if (i < o) continue;
      const int j = p ? i >> lm : 0;
      const int k = PK[(1 << p) - 1 + j];
      if (i == (j ? j << lm : o)) { fe_put(W, (unsigned)k, 4, pos); pos += 4; }
      const unsigned u = U[fe_uidx(i)];
      pos += (int)(u >> k);                                            // the unary zeros are already there
      fe_put(W, (1u << k) | (u & ((1u << k) - 1u)), k + 1, pos);
      pos += k + 1;
    }
  }
  __syncthreads();

  // ---- CRC-16 over the zero-padded frame, then the footer ----
  const int nbody = (total_bits + 7) >> 3;
  const int L = (nbody + FE_THREADS - 1) / FE_THREADS, pad = FE_THREADS * L - nbody;      // right-aligned: leading zeros leave a zero CRC
  unsigned crc = 0;
  for (int jj = 0; jj < L; ++jj) {
    const int pj = t * L + jj;
    if (pj >= pad) {
      crc ^= fe_byte(W, pj - pad) << 8;
#pragma unroll
      for (int b = 0; b < 8; ++b) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x8005u) & 0xffffu : (crc << 1) & 0xffffu;
    }
  }
  unsigned mult = 1;                                                   // x^(8 L)
  for (int b = 0; b < 8 * L; ++b) mult = (mult & 0x8000u) ? ((mult << 1) ^ 0x8005u) & 0xffffu : (mult << 1) & 0xffffu;
  CR[t] = crc;
  for (int s = 1; s < FE_THREADS; s <<= 1) {
    __syncthreads();
    if ((t & (2 * s - 1)) == 0) CR[t] = fe_mulmod16(CR[t], mult) ^ CR[t + s];
    mult = fe_mulmod16(mult, mult);
  }
  __syncthreads();
  if (t == 0) fe_put(W, CR[0], 16, 8 * nbody);
  __syncthreads();
  const int nbytes = nbody + 2;
  unsigned* dst = reinterpret_cast<unsigned*>(slots + f * (int64_t)slot_stride);
  for (int i = t; i < (nbytes + 3) >> 2; i += FE_THREADS) dst[i] = __builtin_bswap32(W[i]);
  if (t == 0) frame_bytes[f] = nbytes;
}

// exclusive prefix of the frame sizes (one workgroup; int64 offsets), off[F] = total
__global__ __launch_bounds__(1024) void flac_frame_offsets_kernel(const int32_t* __restrict__ frame_bytes, int64_t* __restrict__ off, int64_t F) {
  __shared__ long long part[1024];
  const int t = threadIdx.x;
  const int64_t per = (F + 1023) / 1024, a = t * per, b = a + per < F ? a + per : F;
  long long sum = 0;
  for (int64_t i = a; i < b; ++i) sum += frame_bytes[i];
  part[t] = sum;
  __syncthreads();
  for (int s = 1; s < 1024; s <<= 1) {
    const long long v = t >= s ? part[t - s] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  long long run = part[t] - sum;
  for (int64_t i = a; i < b; ++i) { off[i] = run; run += frame_bytes[i]; }
  if (t == 1023) off[F] = part[1023];
}

// the frames of a file, and the files of the batch, back to back
__global__ __launch_bounds__(FE_THREADS) void flac_compact_kernel(const unsigned char* __restrict__ slots, const int32_t* __restrict__ frame_bytes,
                                                                  const int64_t* __restrict__ off, unsigned char* __restrict__ out, int slot_stride) {
  const int64_t f = blockIdx.x;
  const unsigned char* src = slots + f * (int64_t)slot_stride;
  unsigned char* dst = out + off[f];
  const int nb = frame_bytes[f];
  for (int i = threadIdx.x; i < nb; i += FE_THREADS) dst[i] = src[i];
}

__global__ void pcm16_from_f32_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ lens, int16_t* __restrict__ pcm,
                                      int64_t ldp, int max_len, float scale) {
  const int64_t row = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= max_len) return;
  const int len = lens ? lens[row] : max_len;
  float v = 0.f;
  if (i < len) {
    v = rintf(x[row * ldx + i] * scale);                               // round half to even, as numpy.round
    v = v != v ? 0.f : fminf(fmaxf(v, -32768.f), 32767.f);
  }
  pcm[row * ldp + i] = (int16_t)v;
}

static int fe_rate_code(int fs) {
  switch (fs) {
    case 8000: return 4; case 16000: return 5; case 22050: return 6; case 24000: return 7;
    case 32000: return 8; case 44100: return 9; case 48000: return 10; default: return -1;
  }
}
static bool fe_blocksize_ok(int bs) { return bs == 256 || bs == 512 || bs == 1024 || bs == 2048 || bs == 4096; }
static int64_t fe_align(int64_t v) { return (v + 255) / 256 * 256; }

struct FeLayout { int64_t frames, desc, sizes, offs, slots, compact, total; int stride; };
static FeLayout fe_layout(const int32_t* lens, int P, int bs) {
  FeLayout l{};
  for (int p = 0; p < P; ++p) l.frames += (lens[p] + (int64_t)bs - 1) / bs;
  l.stride = 2 * bs + FE_SLOT_EXTRA;
  const int64_t F = l.frames > 0 ? l.frames : 1;
  l.desc = 0;
  l.sizes = fe_align(l.desc + F * (int64_t)sizeof(FlacFrameDesc));
  l.offs = fe_align(l.sizes + F * 4);
  l.slots = fe_align(l.offs + (F + 1) * 8);
  l.compact = fe_align(l.slots + F * l.stride);
  l.total = fe_align(l.compact + F * l.stride);
  return l;
}

}  // namespace urse

using namespace urse;

extern "C" int urse_pcm16_from_f32(const float* x, int64_t ldx, const int32_t* lens, int16_t* pcm, int64_t ldp, int64_t rows,
                                   int max_len, float scale, void* stream) {
  URSE_CHECK_ARG(x && pcm && rows > 0 && max_len > 0, "urse_pcm16_from_f32: bad argument");
  URSE_CHECK_ARG(ldx >= max_len && ldp >= max_len, "urse_pcm16_from_f32: row pitch %ld / %ld below max_len %d", (long)ldx, (long)ldp,
                 max_len);
  for (int64_t r0 = 0; r0 < rows; r0 += 65535) {
    const int64_t nr = rows - r0 < 65535 ? rows - r0 : 65535;
    hipLaunchKernelGGL(pcm16_from_f32_kernel, dim3(ceil_div(max_len, 256), (unsigned)nr), dim3(256), 0, (hipStream_t)stream,
                       x + r0 * ldx, ldx, lens ? lens + r0 : nullptr, pcm + r0 * ldp, ldp, max_len, scale);
  }
  URSE_CHECK_LAUNCH("urse_pcm16_from_f32");
  return URSE_OK;
}

extern "C" int urse_flac_encode_workspace_bytes(const int32_t* lens, int P, int blocksize, int64_t* info) {
  URSE_CHECK_ARG(lens && info && P > 0, "urse_flac_encode_workspace_bytes: bad argument");
  if (!fe_blocksize_ok(blocksize)) {
    set_error("urse_flac_encode_workspace_bytes: block size %d is not one of 256, 512, 1024, 2048, 4096", blocksize);
    return URSE_ERR_UNSUPPORTED;
  }
  for (int p = 0; p < P; ++p) URSE_CHECK_ARG(lens[p] >= 0, "urse_flac_encode_workspace_bytes: file %d has a negative length", p);
  const FeLayout l = fe_layout(lens, P, blocksize);
  info[0] = l.total;
  info[1] = l.frames;
  info[2] = l.frames * l.stride;
  return URSE_OK;
}

extern "C" int urse_flac_encode(const int16_t* pcm, int64_t total_samples, const int64_t* starts, const int32_t* lens,
                                const int32_t* rates, int P, int channels, int bits, int blocksize, void* workspace,
                                int64_t workspace_bytes, void* out, int64_t out_capacity, int64_t* file_bytes,
                                int32_t* frame_bytes, void* stream) {
  URSE_CHECK_ARG(pcm && starts && lens && rates && workspace && out && file_bytes && frame_bytes && P > 0 && total_samples >= 0,
                 "urse_flac_encode: bad argument");
  if (channels != 1 || bits != 16) {
    set_error("urse_flac_encode: %d channel(s) of %d bits: only mono 16-bit streams are encoded", channels, bits);
    return URSE_ERR_UNSUPPORTED;
  }
  if (!fe_blocksize_ok(blocksize)) {
    set_error("urse_flac_encode: block size %d is not one of 256, 512, 1024, 2048, 4096", blocksize);
    return URSE_ERR_UNSUPPORTED;
  }
  for (int p = 0; p < P; ++p) {
    URSE_CHECK_ARG(lens[p] >= 0 && starts[p] >= 0 && starts[p] + lens[p] <= total_samples,
                   "urse_flac_encode: file %d (start %ld, %d samples) leaves the %ld samples given", p, (long)starts[p], lens[p],
                   (long)total_samples);
    if (fe_rate_code(rates[p]) < 0) {
      set_error("urse_flac_encode: file %d: no frame-header code for %d Hz (8000, 16000, 22050, 24000, 32000, 44100, 48000)", p, rates[p]);
      return URSE_ERR_UNSUPPORTED;
    }
  }
  const FeLayout l = fe_layout(lens, P, blocksize);
  URSE_CHECK_ARG(workspace_bytes >= l.total, "urse_flac_encode: workspace of %ld bytes is too small (urse_flac_encode_workspace_bytes: %ld)",
                 (long)workspace_bytes, (long)l.total);
  URSE_CHECK_ARG(l.frames < (1LL << 31), "urse_flac_encode: %ld frames exceed the grid", (long)l.frames);
  for (int p = 0; p < P; ++p) file_bytes[p] = 0;
  if (l.frames == 0) return URSE_OK;
  std::vector<FlacFrameDesc> desc((size_t)l.frames);
  int64_t f = 0;
  for (int p = 0; p < P; ++p)
    for (int64_t s = 0, k = 0; s < lens[p]; s += blocksize, ++k) {
      const int n = (int)(lens[p] - s < blocksize ? lens[p] - s : blocksize);
      desc[(size_t)f++] = FlacFrameDesc{starts[p] + s, n | fe_rate_code(rates[p]) << 16, (int32_t)k};
    }
  char* ws = static_cast<char*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  int32_t* d_sizes = reinterpret_cast<int32_t*>(ws + l.sizes);
  int64_t* d_offs = reinterpret_cast<int64_t*>(ws + l.offs);
  hipError_t e = hipMemcpyAsync(ws + l.desc, desc.data(), desc.size() * sizeof(FlacFrameDesc), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) { set_error("urse_flac_encode: frame table upload: %s", hipGetErrorString(e)); return URSE_ERR_RUNTIME; }
  hipLaunchKernelGGL(flac_encode_frames_kernel, dim3((unsigned)l.frames), dim3(FE_THREADS), 0, st, pcm,
                     reinterpret_cast<const FlacFrameDesc*>(ws + l.desc), reinterpret_cast<unsigned char*>(ws + l.slots), d_sizes, blocksize,
                     l.stride);
  hipLaunchKernelGGL(flac_frame_offsets_kernel, dim3(1), dim3(1024), 0, st, d_sizes, d_offs, l.frames);
  hipLaunchKernelGGL(flac_compact_kernel, dim3((unsigned)l.frames), dim3(FE_THREADS), 0, st, reinterpret_cast<const unsigned char*>(ws + l.slots),
                     d_sizes, d_offs, reinterpret_cast<unsigned char*>(ws + l.compact), l.stride);
  e = hipGetLastError();
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);                                    // the frame table is still being read
    set_error("urse_flac_encode: launch failed: %s", hipGetErrorString(e));
    return URSE_ERR_LAUNCH;
  }
  e = hipMemcpyAsync(frame_bytes, d_sizes, (size_t)l.frames * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { set_error("urse_flac_encode: %s", hipGetErrorString(e)); return URSE_ERR_RUNTIME; }
  int64_t total = 0;
  f = 0;
  for (int p = 0; p < P; ++p) {
    int64_t fb = 0;
    for (int64_t s = 0; s < lens[p]; s += blocksize) fb += frame_bytes[f++];
    file_bytes[p] = fb;
    total += fb;
  }
  if (total > out_capacity) {
    for (int p = 0; p < P; ++p) file_bytes[p] = 0;
    set_error("urse_flac_encode: the streams take %ld bytes, the output buffer holds %ld", (long)total, (long)out_capacity);
    return URSE_ERR_INVALID_ARG;
  }
  e = hipMemcpyAsync(out, ws + l.compact, (size_t)total, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { set_error("urse_flac_encode: %s", hipGetErrorString(e)); return URSE_ERR_RUNTIME; }
  return URSE_OK;
}
