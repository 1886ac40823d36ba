// Wind-noise mixing on the device (simulation/simulate_data_from_param.py wind_noise :129-217): the reference writes the
// speech and the SNR-scaled noise to 16-bit files, runs ffmpeg's `sidechaincompress` (the noise ducks the speech) and `amix` over them, reads
// the 16-bit result back and clips it.  No ffmpeg exists where this library is built or tested: the filter is RESTATED from its published
// definition ("restated, unpinned"), everything the command line leaves out at ffmpeg's defaults (level_in 1, mode
// downward, makeup 1, knee 2.82843, link average, detection rms, mix 1).
//
// Per listed row, float64 throughout (the recurrence, the gain and both 16-bit rounding decisions must come out as in the float64 oracle):
//   c  = 0.9 / max(max|x|, max|v|)                       (1 when both peaks are 0, where the reference divides by zero)
//   xq = Q(c x), vq = Q(c v),  Q(y) = clip(rint(32768 y), -32768, 32767) / 32768      (the temporary files)
//   a  = (vq sc_gain)^2,  S += (a - S) (a > S ? ka : kr)                              (envelope follower on the side chain)
//   g  = 1 below the knee, exp(gain(0.5 ln S) - 0.5 ln S) from it on (cubic Hermite inside the knee, the ratio's line above)
//   m  = 0.5 xq g + 0.5 vq,  mq = Q(m),  mix = mq / c,  noise = vq / c                 (amix of two inputs, the output file)
//   mix = max(mix, ct min(mix)), then mix = min(mix, ct max(mix))                      (the clipper, always on: bool("False") is true)
//   clean speech *= c when the row has no RIR (the reference scales the array the clean target aliases)
//
// One workgroup per row.  The envelope follower is a serial chain of four dependent f64 operations per sample, carried by ONE lane; the
// row moves through LDS in chunks of WIND_CHUNK samples, three in flight: while lane 0 of wave 0 runs the recurrence over chunk k (in
// place: a[t] -> S[t]), waves 1-3 finish chunk k-1 (ln / exp / Hermite, amix, Q, running min / max) and stage chunk k+1 (coalesced loads,
// Q, a).  One __syncthreads per chunk; nothing waits on another workgroup.  A last sweep of the same workgroup applies the clipper.
#include <math.h>

#include "urse_common.h"

// every product and sum below is rounded on its own, as numpy rounds it (a fused multiply-add moves the 16-bit rounding decisions)
#pragma clang fp contract(off)

namespace urse {

constexpr int WIND_CHUNK = 1024;
constexpr int WIND_THREADS = 256;
constexpr int WIND_WORKERS = WIND_THREADS - 64;
constexpr int WIND_NPAR = 8;          // {threshold, ratio, attack ms, release ms, sc_gain, clipping_threshold, fs, has_rir}
constexpr double WIND_KNEE = 2.82843;

__device__ __forceinline__ double wind_q16(double y) { return fmin(fmax(rint(32768.0 * y), -32768.0), 32767.0); }   // (the integer)

__global__ void __launch_bounds__(WIND_THREADS) wind_mix_kernel(float* speech, const float* x, float* __restrict__ noise,
                                                                float* __restrict__ noisy, const int* __restrict__ lens, int B, long ld,
                                                                const int* __restrict__ rows, const double* __restrict__ params,
                                                                double* __restrict__ c_out) {
  __shared__ double aS[3][WIND_CHUNK];          // a[t] as staged, S[t] once the recurrence has passed
  __shared__ int xv[3][WIND_CHUNK];             // the two 16-bit samples of the temporary files: xq in the low half, vq in the high half
  __shared__ float s_peak[4];
  __shared__ int s_min, s_max;
  const int j = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = rows[j];
  if (b < 0 || b >= B) return;
  long len = lens[b];
  if (len > ld) len = ld;
  if (len <= 0) return;
  const long base = (long)b * ld;
  const double* pr = params + (long)j * WIND_NPAR;
  const double threshold = pr[0], ratio = pr[1], attack = pr[2], release = pr[3], sc_gain = pr[4], clip_t = pr[5], fs = pr[6];
  const bool has_rir = pr[7] != 0.0;

  // c: the peaks of both inputs
  float pk = 0.f;
  for (long i = tid; i < len; i += WIND_THREADS) pk = fmaxf(pk, fmaxf(fabsf(x[base + i]), fabsf(noise[base + i])));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o, 64));
  if (lane == 0) s_peak[wave] = pk;
  if (tid == 0) { s_min = 32767; s_max = -32768; }
  __syncthreads();
  pk = fmaxf(fmaxf(s_peak[0], s_peak[1]), fmaxf(s_peak[2], s_peak[3]));
  const double c = pk > 0.f ? 0.9 / (double)pk : 1.0;
  if (tid == 0 && c_out) c_out[j] = c;

  // the compressor's constants
  const double thres = log(threshold);
  const double lin_knee_start = threshold / sqrt(WIND_KNEE), lin_knee_stop = threshold * sqrt(WIND_KNEE);
  const double adj_knee_start = lin_knee_start * lin_knee_start;
  const double knee_start = log(lin_knee_start), knee_stop = log(lin_knee_stop);
  const double compressed_knee_stop = (knee_stop - thres) / ratio + thres;
  const double ka = fmin(1.0, 1.0 / (attack * fs / 4000.0)), kr = fmin(1.0, 1.0 / (release * fs / 4000.0));

  const int nch = (int)((len + WIND_CHUNK - 1) / WIND_CHUNK);
  double S = 0.0;                    // (lane 0 of wave 0)
  int mn = 32767, mx = -32768;       // (workers)
  for (int it = 0; it < nch + 2; ++it) {
    if (wave == 0) {
      const int k = it - 1;
      if (lane == 0 && k >= 0 && k < nch) {
        double* p = aS[k % 3];
        const long left = len - (long)k * WIND_CHUNK;
        const int n8 = (int)(left < WIND_CHUNK ? (left + 7) & ~7L : WIND_CHUNK);      // (the stage pads the last chunk with a = 0)
        for (int t = 0; t < n8; t += 8) {
          double a[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) a[u] = p[t + u];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const double d = a[u] - S;
            S = S + d * (a[u] > S ? ka : kr);
            a[u] = S;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) p[t + u] = a[u];
        }
      }
    } else {
      const int w = tid - 64;
      const int kf = it - 2;
      if (kf >= 0) {                                          // finish chunk kf
        const double* ps = aS[kf % 3];
        const int* pq = xv[kf % 3];
        const long t0 = (long)kf * WIND_CHUNK;
        for (int i = w; i < WIND_CHUNK && t0 + i < len; i += WIND_WORKERS) {
          const double Si = ps[i];
          const int q = pq[i];
          const double xq = (double)(short)(q & 0xffff) / 32768.0, vq = (double)(q >> 16) / 32768.0;
          double g = 1.0;
          if (Si > 0.0 && Si > adj_knee_start) {
            const double slope = 0.5 * log(Si);
            double gain = (slope - thres) / ratio + thres;
            if (WIND_KNEE > 1.0 && slope < knee_stop) {       // cubic Hermite from (knee_start, knee_start), slope 1, to (knee_stop, compressed_knee_stop), slope 1 / ratio
              const double width = knee_stop - knee_start, t = (slope - knee_start) / width;
              const double p0 = knee_start, p1 = compressed_knee_stop, m0 = 1.0 * width, m1 = (1.0 / ratio) * width;
              const double t2 = t * t, t3 = t2 * t;
              const double ct2 = -3.0 * p0 - 2.0 * m0 + 3.0 * p1 - m1, ct3 = 2.0 * p0 + m0 - 2.0 * p1 + m1;
              gain = ct3 * t3 + ct2 * t2 + m0 * t + p0;
            }
            g = exp(gain - slope);
          }
          const double y = xq * g;
          const int mq = (int)wind_q16(0.5 * y + 0.5 * vq);
          mn = mq < mn ? mq : mn;
          mx = mq > mx ? mq : mx;
          noisy[base + t0 + i] = (float)mq;                   // (the last sweep turns the integer into the clipped mix)
          noise[base + t0 + i] = (float)(vq / c);
        }
      }
      if (it < nch) {                                         // stage chunk it
        double* pa = aS[it % 3];
        int* pq = xv[it % 3];
        const long t0 = (long)it * WIND_CHUNK;
        for (int i = w; i < WIND_CHUNK; i += WIND_WORKERS) {
          int xi = 0, vi = 0;
          if (t0 + i < len) {
            xi = (int)wind_q16(c * (double)x[base + t0 + i]);
            vi = (int)wind_q16(c * (double)noise[base + t0 + i]);
          }
          const double sc = (double)vi / 32768.0 * sc_gain;
          pa[i] = sc * sc;
          pq[i] = (xi & 0xffff) | (int)((unsigned)vi << 16);
        }
      }
    }
    __syncthreads();
  }
  // min / max of the 16-bit mixture over the row
  if (wave != 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int a = __shfl_xor(mn, o, 64), d = __shfl_xor(mx, o, 64);
      mn = a < mn ? a : mn;
      mx = d > mx ? d : mx;
    }
    if (lane == 0) { atomicMin(&s_min, mn); atomicMax(&s_max, mx); }
  }
  __syncthreads();
  // the clipper: the lower bound first, the upper bound from the result
  const double mix_min = (double)s_min / 32768.0 / c, mix_max = (double)s_max / 32768.0 / c;
  const double lo = clip_t * mix_min;
  const double hi = clip_t * fmax(mix_max, lo);
  for (long i = tid; i < len; i += WIND_THREADS) {
    const double mix = (double)noisy[base + i] / 32768.0 / c;
    noisy[base + i] = (float)fmin(fmax(mix, lo), hi);
    if (!has_rir) speech[base + i] = (float)(c * (double)speech[base + i]);      // (x may be this very buffer: every read of x is done)
  }
}

}  // namespace urse

extern "C" int urse_wind_chunk(void) { return urse::WIND_CHUNK; }

extern "C" int urse_wind_mix(float* speech, const float* x, float* noise, float* noisy, const int32_t* lens, int B, int64_t ld,
                             const int32_t* rows, int nrows, const double* params, double* c_out, void* stream) {
  URSE_CHECK_ARG(speech && x && noise && noisy && lens && B > 0 && ld > 0 && nrows >= 0 && (nrows == 0 || (rows && params)),
                 "urse_wind_mix: bad argument");
  URSE_CHECK_ARG(nrows <= B, "urse_wind_mix: %d rows listed, the batch has %d (each row at most once)", nrows, B);
  URSE_CHECK_ARG(noisy != x && noise != x && noisy != noise && (const float*)speech != noisy && (const float*)speech != noise,
                 "urse_wind_mix: noisy / noise are rewritten while x is read: they must be buffers of their own (speech may be x)");
  if (nrows == 0) return URSE_OK;
  hipLaunchKernelGGL(urse::wind_mix_kernel, dim3(nrows), dim3(urse::WIND_THREADS), 0, (hipStream_t)stream, speech, x, noise, noisy, lens, B,
                     (long)ld, rows, params, c_out);
  URSE_CHECK_LAUNCH("urse_wind_mix");
  return URSE_OK;
}
