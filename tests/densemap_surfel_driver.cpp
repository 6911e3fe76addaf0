// tests/test_densemap_freeze_cpu.py: loam_velodyne_amd/csrc/densemap_surfel.hpp, the function k_dm_surfels runs per slot, built for the
// host with the host compiler and -ffp-contract=off.  stdin: one voxel per line,
//   leaf_bits ix iy iz min_points ratio_bits n Sx Sy Sz m0 .. m8
// (leaf_bits: the f32 leaf as its 32 bits; ratio_bits: min_planar_ratio as its 32 bits; every other word in decimal).  stdout: one line
// per voxel, the 32-bit words of the six f32 and of the curvature in hex, then 1 / 0: the voxel has a surfel.
#include "densemap_surfel.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstring>

// with the argument "conv": one signed 128-bit integer per line as  neg hi lo  (magnitude = hi * 2^64 + lo); prints the 64 bits of
// dm_i128_to_double of it in hex
static int conv() {
  unsigned neg;
  unsigned long long hi, lo;
  while (scanf("%u %llu %llu", &neg, &hi, &lo) == 3) {
    const loamx::dms_i128 m = (loamx::dms_i128)(((loamx::dms_u128)hi << 64) | lo);
    const double d = loamx::dm_i128_to_double(neg ? -m : m);
    uint64_t w;
    memcpy(&w, &d, 8);
    printf("%016" PRIx64 "\n", w);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "conv")) return conv();
  unsigned leaf_bits, min_points, ratio_bits;
  long long ix, iy, iz;
  unsigned long long v[4], m[9];
  for (;;) {
    if (scanf("%u %lld %lld %lld %u %u", &leaf_bits, &ix, &iy, &iz, &min_points, &ratio_bits) != 6) break;
    for (int k = 0; k < 4; k++)
      if (scanf("%llu", &v[k]) != 1) return 2;
    for (int k = 0; k < 9; k++)
      if (scanf("%llu", &m[k]) != 1) return 2;
    float leaf, ratio;
    memcpy(&leaf, &leaf_bits, 4);
    memcpy(&ratio, &ratio_bits, 4);
    loamx_densemap_surfel_config c;
    c.min_points = min_points;
    c.min_planar_ratio = ratio;
    float six[6], curvature;
    const bool has = loamx::dm_surfel_hd((double)leaf, ix, iy, iz, v[0], v[1], v[2], v[3], m, c, six, curvature);
    for (int k = 0; k < 6; k++) {
      uint32_t w;
      memcpy(&w, &six[k], 4);
      printf("%08" PRIx32 " ", w);
    }
    uint32_t w;
    memcpy(&w, &curvature, 4);
    printf("%08" PRIx32 " %d\n", w, has ? 1 : 0);
  }
  return 0;
}
