// Audio-bandwidth estimation for gfx950: the mean power spectrum of every row of a batch and the decision rule on it.
//
// Replaces, per file, utils/estimate_audio_bandwidth.py:32-49 of the reference: torch.stft (centred, reflect padding,
// periodic Hann, one-sided) -> re^2 + im^2 -> mean over the frames -> the highest bin within `threshold` dB of the peak.
// The [rows, T, F] spectrogram is never written: a workgroup forms its frames from the waveform in LDS, transforms two real
// frames per complex FFT (fft_lds.h) and adds the powers of its frame chunk into an LDS accumulator; the chunks of a row are
// added by a second kernel in chunk order.  No float atomics: the same input gives the same bits on every run.
//
// Frame sizes.  The reference's n_fft = int(0.032 fs) is 256 / 512 / 768 / 1024 / 1536 (radix 4 / 2 / 3 passes of fft_lds.h) at
// five of the seven challenge rates, 705 = 3 * 5 * 47 at 22.05 kHz and 1411 = 17 * 83 at 44.1 kHz.  Two paths exist for such sizes:
//  (a) fft_lds.h's generic O(R^2) butterfly per odd prime factor R (a plan of this file: make_fft_plan stops at the prime 61);
//  (b) Bluestein: the n-point DFT as a circular convolution of length M >= 2n - 1, M the smallest 2-3-5-smooth size
//      (1440 for 705, 2880 for 1411): chirp-multiply, FFT_M, multiply by the transformed chirp, FFT_M again (the inverse through
//      conjugation), chirp-multiply - all in LDS, two frames per complex sequence as everywhere.
// Measured (scripts/time_bandwidth.py, 256 rows x 4 s; table at BW_BLUESTEIN_MIN_PRIME below): (b) is 5.9 x faster at 705 and 22 x
// at 1411, (a) wins up to the prime 13.  Any n_fft <= BW_MAX_NFFT runs on (a) when
// its prime factors are <= BW_MAX_PRIME, and any n_fft <= BW_MAX_BLUESTEIN_N on (b); everything else is URSE_ERR_UNSUPPORTED.
#include <map>
#include <mutex>
#include <vector>
#include <math.h>

#include "fft_lds.h"

namespace urse {

constexpr int BW_MAX_NFFT = 4096;           // path (a), LDS: 28 n + 4 (n / 2 + 1) bytes = 120 KiB at the limit
constexpr int BW_MAX_PRIME = 127;           // largest prime factor path (a) takes
constexpr int BW_MAX_BLUESTEIN_N = 2048;    // path (b): M <= 4096, LDS 24 M + 4 (n / 2 + 1) bytes
// path (b) from this largest prime factor on (A/B switch: URSE_BW_BLUESTEIN_MIN_PRIME; 0 = never).  Measured, 256 rows x 4 s:
//   n_fft (largest prime)  448 (7)  441 (7)  704 (11)  832 (13)  1088 (17)  736 (23)  992 (31)  976 (61)  705 (47)  1411 (83)
//   (a) generic, us          186      260      323       455       1059      1056      2418      9179      4037      25240
//   (b) Bluestein, us        467      467      682       715       1105       579       654       655       684       1135
// (the smooth 1536: 419 us on its own passes, 1157 us through Bluestein).  The O(R^2) butterfly loses from R = 23 on and ties at 17.
constexpr int BW_BLUESTEIN_MIN_PRIME = 19;
constexpr int BW_THREADS = 256;
constexpr int BW_THREADS_BLUESTEIN = 512;
constexpr int BW_TARGET_WGS = 4096;         // frame pairs per workgroup are chosen so that a launch has about this many workgroups
constexpr int BW_MAX_PPC = 32;

struct BwTables {
  int bluestein;      // 0: plan / tw are n_fft's own; 1: they are the convolution length M's
  FftPlan plan;
  float2* tw;         // device, plan.n
  float* win;         // device, n (periodic Hann)                                                    [path (a)]
  float2* cw;         // device, n: chirp e^{-i pi j^2 / n} times the window                          [path (b)]
  float2* chirp;      // device, n: the chirp alone
  float2* bfft;       // device, M: FFT_M of the wrapped conjugate chirp, divided by M
};

static std::mutex g_bw_mu;
static std::map<std::pair<int, int>, BwTables> g_bw_tables;   // (device, n_fft)
static std::once_flag g_bw_lds_once;

// make_fft_plan's factorisation with the generic butterfly allowed up to BW_MAX_PRIME; *largest: the largest prime factor taken
static bool make_bw_plan(int n, FftPlan* p, int* largest = nullptr) {
  if (n < 2 || n > BW_MAX_NFFT) return false;
  p->n = n;
  p->nrad = 0;
  int m = n, big = 1;
  while (m % 4 == 0) { p->radix[p->nrad++] = 4; m /= 4; big = 2; }
  while (m % 2 == 0) { p->radix[p->nrad++] = 2; m /= 2; big = 2; }
  while (m % 3 == 0) { p->radix[p->nrad++] = 3; m /= 3; big = 3; }
  while (m % 5 == 0) { p->radix[p->nrad++] = 5; m /= 5; big = 5; }
  for (int f = 7; f <= BW_MAX_PRIME && m > 1; f += 2)
    while (m % f == 0) { if (p->nrad >= 12) return false; p->radix[p->nrad++] = f; m /= f; big = f; }
  if (m != 1 || p->nrad > 12) return false;
  p->m_n = fastdiv_magic((unsigned)n);
  p->m_f = fastdiv_magic((unsigned)(n / 2 + 1));
  int Ns = 1;
  for (int s = 0; s < p->nrad; ++s) {
    p->m_nb[s] = fastdiv_magic((unsigned)(n / p->radix[s]));
    p->m_ns[s] = fastdiv_magic((unsigned)Ns);
    Ns *= p->radix[s];
  }
  if (largest) *largest = big;
  return true;
}

static int bw_bluestein_min_prime() {
  const char* e = getenv("URSE_BW_BLUESTEIN_MIN_PRIME");
  return e ? atoi(e) : BW_BLUESTEIN_MIN_PRIME;
}

// smallest 2-3-5-smooth M >= 2n - 1
static int bw_bluestein_len(int n) {
  for (int M = 2 * n - 1;; ++M) {
    int m = M;
    while (m % 2 == 0) m /= 2;
    while (m % 3 == 0) m /= 3;
    while (m % 5 == 0) m /= 5;
    if (m == 1) return M;
  }
}

// which path n_fft takes: 0 = (a), 1 = (b), -1 = neither (message set)
static int bw_path(const char* who, int n) {
  FftPlan p;
  int largest = 0;
  const bool direct = make_bw_plan(n, &p, &largest);
  const int minp = bw_bluestein_min_prime();
  const bool blue_ok = n <= BW_MAX_BLUESTEIN_N;
  if (direct && !(blue_ok && minp > 0 && largest >= minp)) return 0;
  if (blue_ok && (minp > 0 || !direct)) return 1;
  if (direct) return 0;
  if (n > BW_MAX_NFFT)
    set_error("%s: n_fft=%d is above the limit of %d", who, n, BW_MAX_NFFT);
  else
    set_error("%s: n_fft=%d is above %d and has a prime factor > %d (or too many factors)", who, n, BW_MAX_BLUESTEIN_N, BW_MAX_PRIME);
  return -1;
}

template <typename T>
static bool bw_upload(T** dst, const std::vector<T>& v) {
  if (hipMalloc(dst, v.size() * sizeof(T)) != hipSuccess) return false;
  return hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
}

static int bw_get_tables(int n, BwTables* out) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(g_bw_mu);
  auto it = g_bw_tables.find({dev, n});
  if (it != g_bw_tables.end()) { *out = it->second; return URSE_OK; }
  const int path = bw_path("urse_power_spectrum_mean", n);
  if (path < 0) return URSE_ERR_UNSUPPORTED;
  BwTables t = {};
  t.bluestein = path;
  const int M = path ? bw_bluestein_len(n) : n;
  if (!make_bw_plan(M, &t.plan)) {
    set_error("urse_power_spectrum_mean: no plan for length %d", M);
    return URSE_ERR_UNSUPPORTED;
  }
  std::vector<float2> tw(M);
  std::vector<double> twr(M), twi(M);
  for (int j = 0; j < M; ++j) {
    const double a = -2.0 * M_PI * (double)j / (double)M;
    twr[j] = cos(a); twi[j] = sin(a);
    tw[j] = make_float2((float)twr[j], (float)twi[j]);
  }
  std::vector<float> w(n);
  for (int j = 0; j < n; ++j) w[j] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)j / (double)n));   // periodic Hann
  bool ok = bw_upload(&t.tw, tw);
  if (!path) {
    ok = ok && bw_upload(&t.win, w);
  } else {
    // chirp c[j] = e^{-i pi j^2 / n}, the angle reduced exactly: j^2 mod 2n
    std::vector<double> cr(n), ci(n);
    std::vector<float2> chirp(n), cw(n), bfft(M);
    for (int j = 0; j < n; ++j) {
      const double a = -M_PI * (double)(((long)j * j) % (2L * n)) / (double)n;
      cr[j] = cos(a); ci[j] = sin(a);
      chirp[j] = make_float2((float)cr[j], (float)ci[j]);
      const double wd = 0.5 - 0.5 * cos(2.0 * M_PI * (double)j / (double)n);
      cw[j] = make_float2((float)(cr[j] * wd), (float)(ci[j] * wd));
    }
    // b[m] = conj c[|m|] wrapped to length M; its DFT in double (2n - 1 non-zero terms per bin), divided by M for the inverse
    for (int k = 0; k < M; ++k) {
      double sr = cr[0], si = -ci[0];
      for (int m = 1; m < n; ++m) {
        // conj c[m] (e^{-2 pi i k m / M} + e^{+2 pi i k m / M}) = conj c[m] * 2 cos(2 pi k m / M)
        const double c2 = 2.0 * twr[(int)(((long)k * m) % M)];
        sr += cr[m] * c2;
        si += -ci[m] * c2;
      }
      bfft[k] = make_float2((float)(sr / M), (float)(si / M));
    }
    ok = ok && bw_upload(&t.chirp, chirp) && bw_upload(&t.cw, cw) && bw_upload(&t.bfft, bfft);
  }
  if (!ok) {
    set_error("urse_power_spectrum_mean: allocation of the plan tables failed");
    return URSE_ERR_RUNTIME;
  }
  g_bw_tables[{dev, n}] = t;
  *out = t;
  return URSE_OK;
}

static size_t bw_lds_bytes(const BwTables& t, int n) {
  return (size_t)t.plan.n * 24 + (t.bluestein ? 0 : (size_t)n * 4) + (size_t)(n / 2 + 1) * 4;
}

// launch geometry, shared by the workspace query and the launch: frame pairs per workgroup and chunks per row
static void bw_geometry(int64_t rows, int max_len, int hop, int* ppc, int* nchunk) {
  const int64_t pairs = ((int64_t)max_len / hop + 2) / 2;        // ceil(T / 2), T = 1 + max_len / hop
  int64_t p = rows * pairs / BW_TARGET_WGS;
  p = p < 1 ? 1 : (p > BW_MAX_PPC ? BW_MAX_PPC : p);
  *ppc = (int)p;
  *nchunk = (int)((pairs + p - 1) / p);
}

// sample i of frame t of a row of `len` samples, reflected at both ends of the row's own length (len > half keeps one
// reflection inside [0, len))
__device__ __forceinline__ int bw_reflect(int t, int hop, int i, int half, int len) {
  int q = t * hop + i - half;
  q = q < 0 ? -q : q;
  return q >= len ? 2 * (len - 1) - q : q;
}

// part f32 [rows, nchunk, F]: the summed power of the chunk's frames.  A row shorter than its reflect padding
// (len <= n / 2, which torch.stft refuses) has no frames: its partial sums are zero.
// BLUE = false: plan is n's own, aux0 = the window.  BLUE = true: plan is the convolution length M's, cw / chirp / bfft as BwTables.
template <bool BLUE>
__global__ void __launch_bounds__(BLUE ? BW_THREADS_BLUESTEIN : BW_THREADS)
bw_power_kernel(const float* __restrict__ x, int64_t ld, const int32_t* __restrict__ lens, float* __restrict__ part, FftPlan plan,
                int n, int hop, int max_len, const float* __restrict__ win_g, const float2* __restrict__ tw_g,
                const float2* __restrict__ cw_g, const float2* __restrict__ chirp_g, const float2* __restrict__ bfft_g, int ppc,
                int nchunk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int M = plan.n, half = n / 2, F = half + 1, nth = blockDim.x;
  float2* tw = reinterpret_cast<float2*>(smem);
  float2* bufA = tw + M;
  float2* bufB = bufA + M;
  float* acc = reinterpret_cast<float*>(bufB + M);
  float* win = acc + F;                      // (path (a) only)
  const int64_t row = blockIdx.x / nchunk;
  const int chunk = blockIdx.x - (int)row * nchunk;
  int len = lens[row];
  len = len > max_len ? max_len : len;
  const int T = len > half ? 1 + (len + 2 * half - n) / hop : 0;   // torch.stft: 1 + (padded - n) / hop; odd n pads n - 1
  const int npairs = (T + 1) / 2;
  const int p0 = chunk * ppc;
  const int p1 = p0 + ppc < npairs ? p0 + ppc : npairs;
  for (int i = threadIdx.x; i < M; i += nth) tw[i] = tw_g[i];
  if (!BLUE)
    for (int i = threadIdx.x; i < n; i += nth) win[i] = win_g[i];
  for (int k = threadIdx.x; k < F; k += nth) acc[k] = 0.f;
  __syncthreads();
  const float* xr = x + row * ld;
  for (int p = p0; p < p1; ++p) {          // workgroup-uniform bounds
    const int ta = 2 * p;
    const bool has_b = ta + 1 < T;
    for (int i = threadIdx.x; i < M; i += nth) {
      float2 z = make_float2(0.f, 0.f);
      if (i < n) {
        const float va = xr[bw_reflect(ta, hop, i, half, len)];
        const float vb = has_b ? xr[bw_reflect(ta + 1, hop, i, half, len)] : 0.f;
        if (BLUE) {
          const float2 c = cw_g[i];
          z = cmul(make_float2(va, vb), c);
        } else {
          const float w = win[i];
          z = make_float2(va * w, vb * w);
        }
      }
      bufA[i] = z;
    }
    __syncthreads();
    const float2* Z = fft_lds_forward(bufA, bufB, 1, plan, tw);
    if (BLUE) {
      // Y = IFFT_M(A .* B) = conj(FFT_M(conj(A .* B))) (1 / M inside B);  Z[k] = chirp[k] * Y[k]: Z is read as chirp * conj(W) below
      float2* A = const_cast<float2*>(Z);
      float2* other = (A == bufA) ? bufB : bufA;
      for (int i = threadIdx.x; i < M; i += nth) {
        const float2 v = cmul(A[i], bfft_g[i]);
        A[i] = make_float2(v.x, -v.y);
      }
      __syncthreads();
      Z = fft_lds_forward(A, other, 1, plan, tw);
    }
    for (int k = threadIdx.x; k < F; k += nth) {
      const int kc = k == 0 ? 0 : n - k;
      float2 zk = Z[k], zc = Z[kc];
      if (BLUE) {
        zk = cmul(chirp_g[k], make_float2(zk.x, -zk.y));
        zc = cmul(chirp_g[kc], make_float2(zc.x, -zc.y));
      }
      // frame a = (zk + conj zc) / 2, frame b = -i (zk - conj zc) / 2
      const float ar = zk.x + zc.x, ai = zk.y - zc.y, br = zk.y + zc.y, bi = zk.x - zc.x;
      const float pa = 0.25f * (ar * ar + ai * ai);
      const float pb = has_b ? 0.25f * (br * br + bi * bi) : 0.f;
      acc[k] += pa + pb;
    }
    __syncthreads();
  }
  float* out = part + ((int64_t)row * nchunk + chunk) * F;
  for (int k = threadIdx.x; k < F; k += nth) out[k] = acc[k];
}

// mean_power[row, k] = (sum over the chunks, in chunk order) / T
__global__ void __launch_bounds__(BW_THREADS) bw_mean_kernel(const float* __restrict__ part, const int32_t* __restrict__ lens,
                                                             float* __restrict__ mean_power, int F, int n, int hop,
                                                             int max_len, int ppc, int nchunk) {
  const int64_t row = blockIdx.y;
  const int k = blockIdx.x * BW_THREADS + threadIdx.x;
  if (k >= F) return;
  int len = lens[row];
  len = len > max_len ? max_len : len;
  const int T = len > n / 2 ? 1 + (len + 2 * (n / 2) - n) / hop : 0;
  const int used = ((T + 1) / 2 + ppc - 1) / ppc;       // chunks that hold frames of this row
  const float* p = part + row * nchunk * F + k;
  float s = 0.f;
  for (int c = 0; c < used; ++c) s += p[(int64_t)c * F];
  mean_power[row * F + k] = T > 0 ? s / (float)T : 0.f;
}

// estimate_audio_bandwidth.py:45-49 for file p = rows [row_start[p], row_start[p + 1]):
//   peak[c] = max_f mean_power[c, f];  min_energy = min_c peak[c] * factor;  bin = the largest i with min_c mean_power[c, i] > min_energy.
// The product and the comparison are made in double, as the reference makes them on its float64 tensors.
__global__ void __launch_bounds__(BW_THREADS) bw_pick_kernel(const float* __restrict__ mean_power,
                                                             const int32_t* __restrict__ row_start,
                                                             int32_t* __restrict__ bin, int F, double factor) {
  __shared__ float redf[BW_THREADS / 64];
  __shared__ int redi[BW_THREADS / 64];
  const int p = blockIdx.x;
  const int r0 = row_start[p], r1 = row_start[p + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (r1 <= r0) {
    if (threadIdx.x == 0) bin[p] = -1;
    return;
  }
  float minpeak = INFINITY;
  for (int c = r0; c < r1; ++c) {
    const float* mp = mean_power + (int64_t)c * F;
    float m = -INFINITY;
    for (int k = threadIdx.x; k < F; k += BW_THREADS) m = fmaxf(m, mp[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __syncthreads();
    if (lane == 0) redf[w] = m;
    __syncthreads();
    float pk = redf[0];
    for (int i = 1; i < BW_THREADS / 64; ++i) pk = fmaxf(pk, redf[i]);
    minpeak = fminf(minpeak, pk);
  }
  const double min_energy = (double)minpeak * factor;
  int best = -1;
  for (int k = threadIdx.x; k < F; k += BW_THREADS) {
    float mn = INFINITY;
    for (int c = r0; c < r1; ++c) mn = fminf(mn, mean_power[(int64_t)c * F + k]);
    if ((double)mn > min_energy) best = k;       // k grows along the loop: the last hit is the thread's largest
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  if (lane == 0) redi[w] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    int b = redi[0];
    for (int i = 1; i < BW_THREADS / 64; ++i) b = redi[i] > b ? redi[i] : b;
    bin[p] = b;
  }
}

}  // namespace urse

using namespace urse;

extern "C" int urse_power_spectrum_workspace_bytes(int64_t rows, int max_len, int n_fft, int hop, int64_t* bytes) {
  URSE_CHECK_ARG(bytes && rows > 0 && max_len > 0 && hop > 0 && n_fft >= 2, "urse_power_spectrum_workspace_bytes: bad argument");
  if (bw_path("urse_power_spectrum_workspace_bytes", n_fft) < 0) return URSE_ERR_UNSUPPORTED;
  int ppc, nchunk;
  bw_geometry(rows, max_len, hop, &ppc, &nchunk);
  *bytes = rows * nchunk * (int64_t)(n_fft / 2 + 1) * (int64_t)sizeof(float);
  return URSE_OK;
}

extern "C" int urse_power_spectrum_mean(const float* wav, int64_t ld, const int32_t* lens, float* mean_power, int64_t rows,
                                        int max_len, int n_fft, int hop, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
  URSE_CHECK_ARG(wav && lens && mean_power && workspace && rows > 0 && max_len > 0 && hop > 0 && n_fft >= 2,
                 "urse_power_spectrum_mean: bad argument");
  URSE_CHECK_ARG(ld >= max_len, "urse_power_spectrum_mean: row pitch %ld below max_len %d", (long)ld, max_len);
  if (bw_path("urse_power_spectrum_mean", n_fft) < 0) return URSE_ERR_UNSUPPORTED;
  const int F = n_fft / 2 + 1;
  int ppc, nchunk;
  bw_geometry(rows, max_len, hop, &ppc, &nchunk);
  URSE_CHECK_ARG(workspace_bytes >= rows * nchunk * (int64_t)F * (int64_t)sizeof(float),
                 "urse_power_spectrum_mean: workspace of %ld bytes is too small (urse_power_spectrum_workspace_bytes)",
                 (long)workspace_bytes);
  URSE_CHECK_ARG(rows * nchunk < (1LL << 31), "urse_power_spectrum_mean: %ld rows x %d chunks exceed the grid",
                 (long)rows, nchunk);
  BwTables tb;
  const int rc = bw_get_tables(n_fft, &tb);
  if (rc) return rc;
  std::call_once(g_bw_lds_once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(bw_power_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(bw_power_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
  });
  float* part = static_cast<float*>(workspace);
  if (tb.bluestein)
    hipLaunchKernelGGL(bw_power_kernel<true>, dim3((unsigned)(rows * nchunk)), dim3(BW_THREADS_BLUESTEIN), bw_lds_bytes(tb, n_fft),
                       (hipStream_t)stream, wav, ld, lens, part, tb.plan, n_fft, hop, max_len, tb.win, tb.tw, tb.cw, tb.chirp, tb.bfft,
                       ppc, nchunk);
  else
    hipLaunchKernelGGL(bw_power_kernel<false>, dim3((unsigned)(rows * nchunk)), dim3(BW_THREADS), bw_lds_bytes(tb, n_fft),
                       (hipStream_t)stream, wav, ld, lens, part, tb.plan, n_fft, hop, max_len, tb.win, tb.tw, tb.cw, tb.chirp, tb.bfft,
                       ppc, nchunk);
  URSE_CHECK_LAUNCH("urse_power_spectrum_mean");
  // rows ride on grid.y in slices of 65535
  for (int64_t r0 = 0; r0 < rows; r0 += 65535) {
    const int64_t nr = rows - r0 < 65535 ? rows - r0 : 65535;
    hipLaunchKernelGGL(bw_mean_kernel, dim3(ceil_div(F, BW_THREADS), (unsigned)nr), dim3(BW_THREADS), 0, (hipStream_t)stream,
                       part + r0 * nchunk * F, lens + r0, mean_power + r0 * F, F, n_fft, hop, max_len, ppc, nchunk);
  }
  URSE_CHECK_LAUNCH("urse_power_spectrum_mean");
  return URSE_OK;
}

extern "C" int urse_bandwidth_pick(const float* mean_power, const int32_t* row_start, int32_t* bin, int P, int F,
                                   double threshold_db, void* stream) {
  URSE_CHECK_ARG(mean_power && row_start && bin && P > 0 && F > 0, "urse_bandwidth_pick: bad argument");
  const double factor = pow(10.0, threshold_db / 10.0);
  hipLaunchKernelGGL(bw_pick_kernel, dim3(P), dim3(BW_THREADS), 0, (hipStream_t)stream, mean_power, row_start, bin, F, factor);
  URSE_CHECK_LAUNCH("urse_bandwidth_pick");
  return URSE_OK;
}
