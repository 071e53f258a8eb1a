// The body of k_cross_spectra, k_cross_spectra_windows and k_cross_spectra_bands (qi_csd.hip), included inside all three:
// what one wave does.  The text is shared as text, not as a function: an inlined callee's __restrict__ scopes reorder
// k_cross_spectra's store epilogue, and that kernel's device code is kept as it was.
// In scope: T, NJ; Z, S (the kernel's arguments); const CsdArgs& a (the panel); int64_t p (tile group, consumed), f (bin of
// the panel), first, len (the segments summed: len of them from `first`), m (matrix of the stack S that is stored);
// weight() -> double, the factor of the finished sums; and the macro CSD_WAVE_LOAD(row, on, out), the one place where the
// kernels differ: csd_load of the contiguous segments first .. first + len - 1 for the first two -- after preprocessing their
// text, and so their device code, is what it was before there was a third -- and csd_load_strided of the segments
// first + k step for the banded kernel, with `step` in its scope.
// The multiply-add chains depend on `len` alone: the k-th segment is the chain's k-th term wherever it lies in the row, and
// a term at or past len is a zero operand whatever the panel holds there.
  using M = Mx<T>;
  using acc = typename M::acc;
  constexpr int V = M::V, STEP = 4 * V;  // segments of one iteration
  const int lane = threadIdx.x & (kWave - 1);
  // item -> tile row ti and its group of up to NJ tiles tj0 .. tj0 + nj - 1, tj0 >= ti: the groups row by row of the upper triangle
  int64_t ti = 0;
  while (p >= csd_row_groups(a.ntile, ti, NJ)) {
    p -= csd_row_groups(a.ntile, ti, NJ);
    ++ti;
  }
  const int64_t tj0 = ti + p * NJ;
  const int nj = (int)(a.ntile - tj0 < NJ ? a.ntile - tj0 : NJ);
  const bool diag0 = tj0 == ti;  // the group's first tile lies on the diagonal: its B operand is the A operand
  const int r = lane & 15, g = lane >> 4;
  // (a record past C: the pointer stays inside the panel, the operand is zero)
  const int64_t ci = ti * kCsdTile + r;
  const bool oni = ci < a.C;
  const cplx<T>* __restrict__ zi = Z + ((oni ? ci : 0) * a.nf + f) * a.nseg + first;
  const cplx<T>* zj[NJ];
  bool onj[NJ];
#pragma unroll
  for (int q = 0; q < NJ; ++q) {
    const int64_t cj = (tj0 + q) * kCsdTile + r;
    onj[q] = q < nj && cj < a.C;
    zj[q] = Z + ((onj[q] ? cj : 0) * a.nf + f) * a.nseg + first;
  }
  acc rr[NJ], ii[NJ], ri[NJ], ir[NJ];
#pragma unroll
  for (int q = 0; q < NJ; ++q) rr[q] = ii[q] = ri[q] = ir[q] = acc{0, 0, 0, 0};
  // one iteration's operands: V segments from `s` of the A record and of the B record of every tile of the group
  auto load = [&](auto check, int64_t s, cplx<T>* x, cplx<T>(*y)[V]) {
    constexpr bool CHECK = decltype(check)::value;
    CSD_WAVE_LOAD(zi, oni, x);
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      if (q >= nj) break;
      if (q > 0 || !diag0) CSD_WAVE_LOAD(zj[q], onj[q], y[q]);
    }
  };
  auto tile_steps = [&](int q, const cplx<T>* x, const cplx<T>* y) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
      rr[q] = M::mac(x[v].x, y[v].x, rr[q]);
      ii[q] = M::mac(x[v].y, y[v].y, ii[q]);
      ri[q] = M::mac(x[v].x, y[v].y, ri[q]);
      ir[q] = M::mac(x[v].y, y[v].x, ir[q]);
    }
  };
  auto steps = [&](const cplx<T>* x, const cplx<T>(*y)[V]) {
    if (diag0) tile_steps(0, x, x);  // the diagonal tile: the A operand's registers twice
    else tile_steps(0, x, y[0]);
#pragma unroll
    for (int q = 1; q < NJ; ++q) {
      if (q >= nj) break;
      tile_steps(q, x, y[q]);
    }
  };
  const int64_t full = len / STEP * STEP, s_lane = g * V;
  cplx<T> xa[V], ya[NJ][V], xb[V], yb[NJ][V];
  int64_t s0 = 0;
  // two iterations' loads are in flight before the first one's products: a wave alone on its SIMD (few records) is bound
  // by the latency of its loads
  for (; s0 + 2 * STEP <= full; s0 += 2 * STEP) {
    load(std::false_type{}, s0 + s_lane, xa, ya);
    load(std::false_type{}, s0 + STEP + s_lane, xb, yb);
    steps(xa, ya);
    steps(xb, yb);
  }
  if (s0 < full) {
    load(std::false_type{}, s0 + s_lane, xa, ya);
    steps(xa, ya);
    s0 += STEP;
  }
  if (s0 < len) {
    load(std::true_type{}, s0 + s_lane, xa, ya);
    steps(xa, ya);
  }
  const T w = (T)weight();
  cplx<T>* __restrict__ Sf = S + m * a.C * a.C;
#pragma unroll
  for (int q = 0; q < NJ; ++q) {
    if (q >= nj) break;
    const bool diag = q == 0 && diag0;
    const int64_t j = (tj0 + q) * kCsdTile + (lane & 15);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t i = ti * kCsdTile + M::row(lane, reg);
      if (i >= a.C || j >= a.C || (diag && j < i)) continue;
      const T re = (rr[q][reg] + ii[q][reg]) * w;
      const T im = i == j ? T(0) : (ri[q][reg] - ir[q][reg]) * w;
      Sf[i * a.C + j] = mk<T>(re, im);
      if (i != j) Sf[j * a.C + i] = mk<T>(re, -im);
    }
  }
