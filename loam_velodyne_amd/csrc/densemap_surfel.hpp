// The surfel of one voxel from its integer words (include/loamx.h, "Second moments and surfels"), as one function for the host and the
// device: the restatement of dm_surfel in axes 0 (densemap_export.hip) and of jacobi_eig3 (host_math.h) that k_dm_surfels
// (densemap_freeze.hip) runs per slot.  Standard library only: tests/test_densemap_freeze_cpu.py builds it with the host compiler and
// holds its bytes to loamx_densemap_surfel_of.
//
// Every output byte equals dm_surfel's.  The arithmetic is f64 + - * / sqrt fabs, comparisons, integer -> double conversions and one
// f64 -> f32 rounding per output, in dm_surfel's order, built without contraction: each of these is correctly rounded on either side,
// so the results do not depend on where the function runs.  The one conversion without a hardware form, 128-bit integer -> double, is
// written out (dm_i128_to_double: round to nearest, ties to even, which is what the host's conversion does).
//
// Registers: the three (p, q) rotations of a Jacobi sweep are written out and the matrices are scalars, so nothing is indexed at run
// time and nothing goes to scratch.
#pragma once
#include "../../include/loamx.h"
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define DMS_HD __host__ __device__
#else
#define DMS_HD
#endif

namespace loamx {

typedef unsigned __int128 dms_u128;
typedef __int128 dms_i128;

// a signed 128-bit integer as the nearest double, ties to even: sign and magnitude; the magnitude's leading 64 bits with a sticky bit
// for what was shifted out (far below the 53rd bit, so the one rounding of the 64-bit conversion is the rounding of the whole), then
// an exact scaling by a power of two.  |v| < 2^127
DMS_HD inline double dm_i128_to_double(dms_i128 v) {
  const bool neg = v < 0;
  const dms_u128 m = neg ? (dms_u128)0 - (dms_u128)v : (dms_u128)v;
  const unsigned long long hi = (unsigned long long)(m >> 64), lo = (unsigned long long)m;
  double r;
  if (hi == 0ull) {
    r = (double)lo;
  } else {
    const int s = 64 - __builtin_clzll(hi);   // 1 .. 64: the bits of the magnitude above the low word
    unsigned long long top = (unsigned long long)(m >> s);
    if ((m & ((((dms_u128)1) << s) - 1)) != 0) top |= 1ull;
    const unsigned long long scale_bits = (unsigned long long)(1023 + s) << 52;   // 2^s
    double scale;
    memcpy(&scale, &scale_bits, sizeof(scale));
    r = (double)top * scale;
  }
  return neg ? -r : r;
}

// One Jacobi rotation of jacobi_eig3 for the pair (p, q) with r the third index: app, aqq the two diagonal elements, apq the element
// it annihilates, arp, arq the two others; (v0p, v0q), (v1p, v1q), (v2p, v2q) the columns p and q of v
DMS_HD inline void dm_jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q, double& v1p,
                                    double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
  const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
  const double a = apq;
  app -= t * a;
  aqq += t * a;
  apq = 0.0;
  const double nrp = c * arp - s * arq, nrq = s * arp + c * arq;
  arp = nrp;
  arq = nrq;
  double vp = v0p, vq = v0q;
  v0p = c * vp - s * vq; v0q = s * vp + c * vq;
  vp = v1p; vq = v1q;
  v1p = c * vp - s * vq; v1q = s * vp + c * vq;
  vp = v2p; vq = v2q;
  v2p = c * vp - s * vq; v2q = s * vp + c * vq;
}

DMS_HD inline void dm_swap2(double& a, double& b) { const double t = a; a = b; b = t; }

// leaf: the voxel's edge; ix, iy, iz: its indices; n, Sx, Sy, Sz and m9: its thirteen words; c: checked settings.  six: mean x, y, z
// and normal x, y, z as dm_surfel gives them in axes 0; curvature: its curvature.  Returns whether the voxel has a surfel (a non-zero
// normal in f32: what the snapshot keeps)
DMS_HD inline bool dm_surfel_hd(double leaf, long long ix, long long iy, long long iz, unsigned long long n, unsigned long long Sx,
                                unsigned long long Sy, unsigned long long Sz, const unsigned long long m9[9],
                                const loamx_densemap_surfel_config& c, float six[6], float& curvature) {
  // the exported position (dm_position)
  const double cnt = (double)n, qs = (double)(1u << 20);
  six[0] = (float)(((double)ix + (double)Sx / (cnt * qs)) * leaf);
  six[1] = (float)(((double)iy + (double)Sy / (cnt * qs)) * leaf);
  six[2] = (float)(((double)iz + (double)Sz / (cnt * qs)) * leaf);
  double n0 = 0.0, n1 = 0.0, n2 = 0.0, curv = 0.0;
  // the scatter n * M_ab - S_a * S_b, exact
  const dms_i128 Nxx = (dms_i128)n * (dms_i128)m9[0] - (dms_i128)Sx * (dms_i128)Sx, Nyy = (dms_i128)n * (dms_i128)m9[1] - (dms_i128)Sy * (dms_i128)Sy,
                 Nzz = (dms_i128)n * (dms_i128)m9[2] - (dms_i128)Sz * (dms_i128)Sz, Nxy = (dms_i128)n * (dms_i128)m9[3] - (dms_i128)Sx * (dms_i128)Sy,
                 Nxz = (dms_i128)n * (dms_i128)m9[4] - (dms_i128)Sx * (dms_i128)Sz, Nyz = (dms_i128)n * (dms_i128)m9[5] - (dms_i128)Sy * (dms_i128)Sz;
  if (n >= c.min_points && Nxx + Nyy + Nzz > 0) {
    const double nn = (double)n * (double)n;
    double a00 = dm_i128_to_double(Nxx) / nn, a11 = dm_i128_to_double(Nyy) / nn, a22 = dm_i128_to_double(Nzz) / nn;
    double a01 = dm_i128_to_double(Nxy) / nn, a02 = dm_i128_to_double(Nxz) / nn, a12 = dm_i128_to_double(Nyz) / nn;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < 32; sweep++) {
      const double off = std::fabs(a01) + std::fabs(a02) + std::fabs(a12);
      const double diag = std::fabs(a00) + std::fabs(a11) + std::fabs(a22);
      if (off == 0.0 || off <= 1e-300 + diag * 1e-22) break;
      dm_jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), third index 2
      dm_jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), third index 1
      dm_jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), third index 0
    }
    // ascending eigenvalues, ties keep the index order: jacobi_eig3's three compare-and-swaps, on the values and their columns
    if (a11 < a00) { dm_swap2(a00, a11); dm_swap2(v00, v01); dm_swap2(v10, v11); dm_swap2(v20, v21); }
    if (a22 < a11) { dm_swap2(a11, a22); dm_swap2(v01, v02); dm_swap2(v11, v12); dm_swap2(v21, v22); }
    if (a11 < a00) { dm_swap2(a00, a11); dm_swap2(v00, v01); dm_swap2(v10, v11); dm_swap2(v20, v21); }
    if (a11 >= (double)c.min_planar_ratio * a22) {
      const double dot = (v00 * (double)(long long)m9[6] + v10 * (double)(long long)m9[7]) + v20 * (double)(long long)m9[8];
      bool flip = dot > 0.0;
      if (dot == 0.0) {
        const double first = v00 != 0.0 ? v00 : (v10 != 0.0 ? v10 : v20);
        flip = first < 0.0;
      }
      n0 = (flip ? -v00 : v00) + 0.0;   // (+ 0.0: no negative zero in the output)
      n1 = (flip ? -v10 : v10) + 0.0;
      n2 = (flip ? -v20 : v20) + 0.0;
      curv = a00 / ((a00 + a11) + a22);
    }
  }
  six[3] = (float)n0; six[4] = (float)n1; six[5] = (float)n2;
  curvature = (float)curv;
  return !(six[3] == 0.f && six[4] == 0.f && six[5] == 0.f);
}

}  // namespace loamx
