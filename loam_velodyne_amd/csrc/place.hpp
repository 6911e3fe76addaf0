// Place recognition (include/loamx.h, loamx_place_*): scan-context descriptors of sweeps in HBM and the exhaustive search over them.
// An entry is R x S f32 cells (the maximum height per ring x sector cell, ring-major; 0 = empty) and R f32 ring-key words.  Heights are
// positive, so their bit patterns order like unsigned integers: the cells are built with integer atomicMax and do not depend on the
// order of the points.
#pragma once
#include "common.h"

namespace loamx {

constexpr int PL_MAX_RINGS = 64;
constexpr int PL_MAX_SECTORS = 128;
constexpr int PL_MAX_CANDIDATES = 256;                 // K of the ring-key pre-selection
constexpr uint32_t PL_CHUNK = 2048;                    // keys per workgroup of a selection pass
constexpr uint32_t PL_DESCRIBE_SPAN = 1024;            // points per workgroup of k_pl_describe (one flush of the LDS grid per span)
constexpr unsigned long long PL_NO_KEY = ~0ull;
constexpr uint32_t PL_FILE_MAGIC = 0x4c50584cu;        // 'LXPL'
constexpr uint32_t PL_FILE_VERSION = 1u;

// boundary directions of the sectors, (cos, sin)(2 pi k / S) evaluated in double and rounded once (host only)
inline void place_sector_table(int S, float* table) {
  const double two_pi = 2.0 * 3.14159265358979323846;
  for (int k = 0; k < S; k++) {
    const double t = two_pi * (double)k / (double)S;
    table[2 * k] = (float)cos(t);
    table[2 * k + 1] = (float)sin(t);
  }
}

}  // namespace loamx
