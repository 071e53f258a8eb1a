// The hipFFT engine of the short-time Fourier family: the kernels around the batched transform, for the geometries the fused
// kernels (qi_stft_fused.hip) do not take.  Forward: frames -> hipFFT -> transpose (or the Welch mean); inverse:
// untranspose -> hipFFT -> overlap-add.  The forward kernels read a StftRequest, as launch_stft_fused does: scipy.signal.stft
// (segment m covers the zero-extended record from m hop - seg / 2, mean removed), Welch (no extension) and
// scipy.signal.ShortTimeFFT (utilities/short_time_fft.py: slice p covers the padded record from p hop - seg // 2; the record is
// extended by zeros, its edge values, or its even / odd reflection; optional detrend; the slice rotated) are requests of one
// framing kernel.  The inverse multiplies the inverse transforms of the slices by the dual window and overlap-adds them: every
// output sample gathers its <= ceil(seg / hop) contributions in slice order (no atomics).
#include "qi_common.hpp"
#include "qi_device.hpp"
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK

namespace qi {

namespace {

// sample k of the record extended past its ends by at most n - 1 samples (np.pad: constant 0 / edge / reflect with
// reflect_type even / odd)
template <typename T>
__device__ __forceinline__ T padded_sample(const T* __restrict__ x, int64_t n, int64_t k, int mode) {
  if (k >= 0 && k < n) return x[k];
  if (mode == 0) return T(0);
  if (mode == 1) return k < 0 ? x[0] : x[n - 1];
  const int64_t j = k < 0 ? -k : 2 * (n - 1) - k;  // mirrored about the end sample (not repeated)
  if (mode == 2) return x[j];
  return T(2) * (k < 0 ? x[0] : x[n - 1]) - x[j];  // point-symmetric about the end value
}

// One workgroup per (segment, channel): the extended segment, its mean removed when asked for (a double sum over the segment
// divided by seg: the extension counts), windowed, zero-padded to nfft.  Rows of `stride` samples, the first n the record's.
template <typename T>
__global__ void __launch_bounds__(256) k_hipfft_frames(const T* __restrict__ sig, const T* __restrict__ win,
                                                       T* __restrict__ frames, int64_t n, int64_t stride, int64_t seg,
                                                       int64_t hop, int64_t nfft, int64_t nseg, int64_t lead, int pad_mode,
                                                       int detrend, int64_t roll) {
  __shared__ double s[256 / kWave];
  __shared__ double s_mean;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const int64_t m = blockIdx.x, c = blockIdx.y;
  const int64_t base = m * hop - lead;  // record index of the segment's first sample (negative before the record)
  const T* x = sig + c * stride;
  T mean = T(0);
  if (detrend) {
    double acc = 0.0;
    for (int64_t i = tid; i < seg; i += 256) acc += (double)padded_sample<T>(x, n, base + i, pad_mode);
    acc = wave_sum(acc);
    if (lane == 0) s[wv] = acc;
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int w = 0; w < 256 / kWave; ++w) t += s[w];
      s_mean = t / (double)seg;
    }
    __syncthreads();
    mean = (T)s_mean;
  }
  // the frame is rotated left by `roll` (ShortTimeFFT's phase_shift convention: with roll = seg // 2 the window centre sits
  // at index 0 of the transform)
  T* f = frames + (c * nseg + m) * nfft;
  for (int64_t i = tid; i < nfft; i += 256) {
    const T v = i < seg ? (padded_sample<T>(x, n, base + i, pad_mode) - mean) * win[i] : T(0);
    int64_t d = i - roll;
    if (d < 0) d += nfft;
    f[d] = v;
  }
}

// F [C * nseg][nf] -> [C][nf][nseg] (frequency x time as the reference returns it), scaled: the complex coefficients into Z
// and / or a real panel of them into R (kind 0: log2(|z| + eps), 1: |z|, 2: |z|^2)
template <typename T>
__global__ void k_hipfft_transpose(const cplx<T>* __restrict__ F, cplx<T>* __restrict__ Z, T* __restrict__ R, int kind,
                                   int64_t nseg, int64_t nf, T scale, T eps) {
  __shared__ cplx<T> tile[32][33];
  const int64_t c = blockIdx.z;
  const int64_t f0 = (int64_t)blockIdx.x * 32, m0 = (int64_t)blockIdx.y * 32;
  for (int r = threadIdx.y; r < 32; r += blockDim.y) {
    int64_t m = m0 + r, f = f0 + threadIdx.x;
    if (m < nseg && f < nf) tile[r][threadIdx.x] = F[(c * nseg + m) * nf + f];
  }
  __syncthreads();
  for (int r = threadIdx.y; r < 32; r += blockDim.y) {
    int64_t f = f0 + r, m = m0 + threadIdx.x;
    if (m < nseg && f < nf) {
      cplx<T> z = tile[threadIdx.x][r];
      z.x *= scale;
      z.y *= scale;
      if (Z) Z[(c * nf + f) * nseg + m] = z;
      if (R) {
        const T p = z.x * z.x + z.y * z.y;
        R[(c * nf + f) * nseg + m] = kind == 2 ? p : (kind == 1 ? sqrt_t(p) : log2_t(sqrt_t(p) + eps));
      }
    }
  }
}

// Welch: Pxx[c][f] = w_f * scale^2 * mean over segments of |F[c][m][f]|^2, w_f = 2 except at DC and (even nfft) Nyquist
// (scipy.signal.welch, scaling="spectrum", average="mean", one-sided; call site styx_fft.py:253-266).
template <typename T>
__global__ void k_welch_mean(const cplx<T>* __restrict__ F, T* __restrict__ pxx, int64_t nseg, int64_t nf, int64_t nfft,
                             T scale2) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (f >= nf) return;
  double acc = 0.0;
  for (int64_t m = 0; m < nseg; ++m) {
    const cplx<T> z = F[(c * nseg + m) * nf + f];
    acc += (double)(z.x * z.x + z.y * z.y);
  }
  const bool paired = f > 0 && !(nfft % 2 == 0 && f == nf - 1);
  pxx[c * nf + f] = (T)(acc / (double)nseg) * scale2 * (paired ? T(2) : T(1));
}

// S [C][nf][nseg] -> F [C * nseg][nf] (slice-major, what the batched inverse transform reads)
template <typename T>
__global__ void k_sliding_untranspose(const cplx<T>* __restrict__ S, cplx<T>* __restrict__ F, int64_t nseg, int64_t nf) {
  __shared__ cplx<T> tile[32][33];
  const int64_t c = blockIdx.z;
  const int64_t m0 = (int64_t)blockIdx.x * 32, f0 = (int64_t)blockIdx.y * 32;
  for (int r = threadIdx.y; r < 32; r += blockDim.y) {
    int64_t f = f0 + r, m = m0 + threadIdx.x;
    if (m < nseg && f < nf) tile[r][threadIdx.x] = S[(c * nf + f) * nseg + m];
  }
  __syncthreads();
  for (int r = threadIdx.y; r < 32; r += blockDim.y) {
    int64_t m = m0 + r, f = f0 + threadIdx.x;
    if (m < nseg && f < nf) F[(c * nseg + m) * nf + f] = tile[threadIdx.x][r];
  }
}

// x[k] = sum over the slices q that cover k of slice_q[k - (first + q hop)] * dual[k - (first + q hop)], k0 <= k < k1;
// `first` is the record index of slice 0's first sample; the unnormalised inverse transform is scaled by 1 / nfft.
template <typename T>
__global__ void __launch_bounds__(256) k_sliding_overlap_add(const T* __restrict__ slices, const T* __restrict__ dual,
                                                             T* __restrict__ out, int64_t k0, int64_t k1, int64_t seg,
                                                             int64_t hop, int64_t nfft, int64_t nseg, int64_t first,
                                                             int64_t roll) {
  const int64_t c = blockIdx.y;
  const T inv = T(1) / (T)nfft;
  for (int64_t k = k0 + (int64_t)blockIdx.x * 256 + threadIdx.x; k < k1; k += (int64_t)gridDim.x * 256) {
    // slices with first + q hop <= k < first + q hop + seg
    int64_t q_hi = (k - first) / hop;
    if (k - first < 0) q_hi = -1;
    int64_t q_lo = (k - first - seg) / hop + 1;
    if (k - first - seg < 0) q_lo = 0;
    if (q_hi > nseg - 1) q_hi = nseg - 1;
    T acc = T(0);
    for (int64_t q = q_lo; q <= q_hi; ++q) {
      const int64_t i = k - (first + q * hop);
      int64_t d = i - roll;  // undo the rotation of the forward transform
      if (d < 0) d += nfft;
      acc += slices[(c * nseg + q) * nfft + d] * dual[i];
    }
    out[c * (k1 - k0) + (k - k0)] = acc * inv;
  }
}

}  // namespace

template <typename T>
int launch_hipfft_frames(const StftRequest& rq, const T* sig, const T* win, T* frames, hipStream_t st) {
  k_hipfft_frames<T><<<dim3((unsigned)rq.nseg, (unsigned)rq.C), 256, 0, st>>>(
      sig, win, frames, rq.n, rq.row_stride < 0 ? rq.n : rq.row_stride, rq.seg, rq.hop, rq.nfft, rq.nseg, rq.lead, rq.pad_mode,
      rq.detrend, rq.roll);
  QI_LAUNCH_CHECK();
  return QI_OK;
}

template <typename T>
int launch_hipfft_transpose(const StftRequest& rq, const cplx<T>* F, cplx<T>* Z, T* R, hipStream_t st) {
  const int64_t nf = rq.nfft / 2 + 1;
  dim3 g((unsigned)ceil_div(nf, 32), (unsigned)ceil_div(rq.nseg, 32), (unsigned)rq.C);
  k_hipfft_transpose<T><<<g, dim3(32, 8), 0, st>>>(F, Z, R, rq.real_kind, rq.nseg, nf, (T)rq.scale, (T)rq.eps);
  QI_LAUNCH_CHECK();
  return QI_OK;
}

template <typename T>
int launch_welch_mean(const StftRequest& rq, const cplx<T>* F, T* pxx, hipStream_t st) {
  const int64_t nf = rq.nfft / 2 + 1;
  dim3 g((unsigned)ceil_div(nf, 256), (unsigned)rq.C);
  k_welch_mean<T><<<g, 256, 0, st>>>(F, pxx, rq.nseg, nf, rq.nfft, (T)(rq.scale * rq.scale));
  QI_LAUNCH_CHECK();
  return QI_OK;
}

template <typename T>
int launch_sliding_untranspose(const cplx<T>* S, cplx<T>* F, int64_t C, int64_t nseg, int64_t nf, hipStream_t st) {
  dim3 g((unsigned)ceil_div(nseg, 32), (unsigned)ceil_div(nf, 32), (unsigned)C);
  k_sliding_untranspose<T><<<g, dim3(32, 8), 0, st>>>(S, F, nseg, nf);
  QI_LAUNCH_CHECK();
  return QI_OK;
}

template <typename T>
int launch_sliding_overlap_add(const T* slices, const T* dual, T* out, int64_t C, int64_t k0, int64_t k1, int64_t seg,
                               int64_t hop, int64_t nfft, int64_t nseg, int64_t first, int64_t roll, hipStream_t st) {
  const int64_t g = ceil_div(k1 - k0, 256);
  k_sliding_overlap_add<T><<<dim3((unsigned)(g > 4096 ? 4096 : (g < 1 ? 1 : g)), (unsigned)C), 256, 0, st>>>(
      slices, dual, out, k0, k1, seg, hop, nfft, nseg, first, roll);
  QI_LAUNCH_CHECK();
  return QI_OK;
}

#define QI_INSTANTIATE_STFT_HIPFFT(T)                                                                             \
  template int launch_hipfft_frames<T>(const StftRequest&, const T*, const T*, T*, hipStream_t);                         \
  template int launch_hipfft_transpose<T>(const StftRequest&, const cplx<T>*, cplx<T>*, T*, hipStream_t);                \
  template int launch_welch_mean<T>(const StftRequest&, const cplx<T>*, T*, hipStream_t);                         \
  template int launch_sliding_untranspose<T>(const cplx<T>*, cplx<T>*, int64_t, int64_t, int64_t, hipStream_t);   \
  template int launch_sliding_overlap_add<T>(const T*, const T*, T*, int64_t, int64_t, int64_t, int64_t, int64_t, \
                                             int64_t, int64_t, int64_t, int64_t, hipStream_t);
QI_INSTANTIATE_STFT_HIPFFT(float)
QI_INSTANTIATE_STFT_HIPFFT(double)

}  // namespace qi
