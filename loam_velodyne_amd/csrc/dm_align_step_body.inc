// The body of the two step kernels of densemap_align.hip, included textually in each (so that both compile from one text and the single
// step keeps its instruction stream): one block's 256 points linearised about the pose A.  In scope: pts, n, A (DmAlign), tab, mask,
// shift and acc, the 33 words of this pose.
// acc: [0, 28) the sums (two's complement), [28, 33) far, outside, unmatched, rejected, matched.  f32, no fused multiply-add (the
// file is built without contraction): the expressions are those of include/loamx.h, in its order
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63), wid = (int)(threadIdx.x >> 6);
  int cls = -1;   // the counter this point goes to (-1: no point)
  long long s[DM_ALIGN_SUMS];
#pragma unroll
  for (int k = 0; k < DM_ALIGN_SUMS; k++) s[k] = 0ll;
  if (i < n) {
    const float4 p = pts[i];
    const float dx = p.x - A.c[0], dy = p.y - A.c[1], dz = p.z - A.c[2];
    float a[3], pp[3], fi[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      a[k] = (A.R[3 * k] * dx + A.R[3 * k + 1] * dy) + A.R[3 * k + 2] * dz;
      pp[k] = a[k] + A.t[k];
      fi[k] = floorf(pp[k] * A.inv);
    }
    if (!(fabsf(a[0]) < DM_ALIGN_FAR && fabsf(a[1]) < DM_ALIGN_FAR && fabsf(a[2]) < DM_ALIGN_FAR)) {
      cls = 0;   // (NaN too)
    } else if (!(fabsf(fi[0]) < DM_IMAX && fabsf(fi[1]) < DM_IMAX && fabsf(fi[2]) < DM_IMAX)) {
      cls = 1;
    } else {
      const int ic[3] = {(int)fi[0], (int)fi[1], (int)fi[2]};
      const int lim = 1 << DM_QBITS;
      bool found = false;
      float best = 0.f, e[3] = {0.f, 0.f, 0.f};
      uint32_t at = 0u;
      for (int oz = -A.nb; oz <= A.nb; oz++)
        for (int oy = -A.nb; oy <= A.nb; oy++)
          for (int ox = -A.nb; ox <= A.nb; ox++) {
            const int cx = ic[0] + ox, cy = ic[1] + oy, cz = ic[2] + oz;
            if (cx <= -lim || cx >= lim || cy <= -lim || cy >= lim || cz <= -lim || cz >= lim) continue;   // outside the key range
            uint32_t slot = 0u;
            float mx = 0.f, my = 0.f;
            if (!dm_frozen_find(tab, mask, shift, dm_key(cx, cy, cz), slot, mx, my)) continue;
            const float ex = pp[0] - mx, ey = pp[1] - my, ez = pp[2] - tab[slot].mean[2];
            const float d2 = (ex * ex + ey * ey) + ez * ez;
            if (!found || d2 < best) {
              found = true; best = d2; at = slot;
              e[0] = ex; e[1] = ey; e[2] = ez;
            }
          }
      if (!found) {
        cls = 2;
      } else {
        const float4 w = *(const float4*)&tab[at].mean[2];   // mean z and the normal: the entry's second 16 bytes
        const float nx = w.y, ny = w.z, nz = w.w;
        const float r = (nx * e[0] + ny * e[1]) + nz * e[2];
        if (!(fabsf(r) <= A.max_residual)) {
          cls = 3;
        } else {
          cls = 4;
          const float J[6] = {a[1] * nz - a[2] * ny, a[2] * nx - a[0] * nz, a[0] * ny - a[1] * nx, nx, ny, nz};
          int w_ = 0;
#pragma unroll
          for (int k = 0; k < 6; k++)
#pragma unroll
            for (int l = k; l < 6; l++) s[w_++] = (long long)rintf((J[k] * J[l]) * DM_ALIGN_HSCALE);
#pragma unroll
          for (int k = 0; k < 6; k++) s[21 + k] = (long long)rintf((J[k] * r) * DM_ALIGN_GSCALE);
          s[27] = (long long)rintf((r * r) * DM_ALIGN_GSCALE);
        }
      }
    }
  }
  __shared__ unsigned long long part[4][DM_ALIGN_WORDS];
  const bool any_matched = __ballot(cls == 4) != 0ull;   // (wave-uniform: a wave without a match has nothing but zeros to sum)
#pragma unroll
  for (int k = 0; k < DM_ALIGN_SUMS; k++) {
    const unsigned long long v = any_matched ? dm_wave_sum_u64((unsigned long long)s[k]) : 0ull;
    if (lane == 0) part[wid][k] = v;
  }
#pragma unroll
  for (int k = 0; k < DM_ALIGN_COUNTS; k++) {
    const unsigned long long m = __ballot(cls == k);
    if (lane == 0) part[wid][DM_ALIGN_SUMS + k] = (unsigned long long)__popcll(m);
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)DM_ALIGN_WORDS) {
    const unsigned long long v = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
    if (v) atomicAdd(&acc[threadIdx.x], v);   // (integer, modulo 2^64: the order does not matter)
  }
