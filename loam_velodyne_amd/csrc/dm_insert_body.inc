// The body of the insert kernels of densemap.hip, included textually in each (so that both compile from one text and k_dm_insert keeps
// its instruction stream): one point per thread goes into the table.  In scope: lane, wid, F (DmFilter: the range filter about the
// point's origin), keys, vals, mask, shift, ctr, aux, seq, mom, the template switches COMBINE, STAMP, MOMENTS and two macros:
// DM_INSERT_HAS_POINT, true when this thread has a point, and DM_INSERT_POINT, that point as a float4
  unsigned long long key = DM_EMPTY;
  uint32_t q[3] = {0u, 0u, 0u};
  int w[3] = {0, 0, 0};   // (MOMENTS) the fixed-point vector from the origin
  bool drop_range = false, drop_key = false;
  if (DM_INSERT_HAS_POINT) {
    const float4 p = DM_INSERT_POINT;
    const float dx = p.x - F.ox, dy = p.y - F.oy, dz = p.z - F.oz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    if (!(d2 >= F.min2 && (!F.use_max || d2 <= F.max2))) {
      drop_range = true;
    } else {
      const float c[3] = {p.x, p.y, p.z};
      unsigned long long k = 0ull;
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const float t = c[a] * F.inv;
        const float fi = floorf(t);
        if (!(fabsf(fi) < DM_IMAX)) drop_key = true;   // (NaN too)
        const float f = t - fi;
        const uint32_t qa = (uint32_t)(f * DM_QSCALE);
        q[a] = drop_key ? 0u : (qa < (1u << DM_QBITS) - 1u ? qa : (1u << DM_QBITS) - 1u);
        const uint32_t ia = drop_key ? 0u : (uint32_t)((int)fi + (1 << DM_QBITS));
        k |= (unsigned long long)ia << (DM_KBITS * a);
      }
      if (!drop_key) key = k;
      if (MOMENTS) {
        const float d[3] = {dx, dy, dz};
#pragma unroll
        for (int a = 0; a < 3; a++) w[a] = (int)fminf(fmaxf(d[a] * 1024.0f, -1073741824.0f), 1073741824.0f);
      }
    }
  }
  dm_wave_count(&ctr[1], drop_range);
  dm_wave_count(&ctr[2], drop_key);
  const bool valid = key != DM_EMPTY;
  uint32_t cnt = valid ? 1u : 0u;
  bool owner = valid;
  unsigned long long ms[DM_MOM_WORDS] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};   // (constant indices only: registers)
  if (MOMENTS) {
    const unsigned long long qx = q[0], qy = q[1], qz = q[2];
    ms[0] = qx * qx; ms[1] = qy * qy; ms[2] = qz * qz;
    ms[3] = qx * qy; ms[4] = qx * qz; ms[5] = qy * qz;
#pragma unroll
    for (int a = 0; a < 3; a++) ms[6 + a] = (unsigned long long)(long long)w[a];
  }
  if (COMBINE) {
    // group the lanes by key: the lowest lane of each group (its leader) collects the group's count and sums
    int leader = -1;
    unsigned long long todo = __ballot(valid);
    while (todo) {
      const int src = __builtin_ctzll(todo);
      const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)key, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(key >> 32), src, 64);
      const unsigned long long k0 = ((unsigned long long)hi << 32) | lo;
      const unsigned long long m = __ballot(valid && key == k0);
      if (valid && key == k0) {
        leader = src;
        if (lane == src) cnt = (uint32_t)__popcll(m);
      }
      todo &= ~m;
    }
    owner = valid && leader == lane;
    if constexpr (MOMENTS) {
      __shared__ unsigned long long macc[4][DM_MOM_WORDS][64];
      if (owner) {
#pragma unroll
        for (int k = 0; k < DM_MOM_WORDS; k++) macc[wid][k][lane] = 0ull;
      }
      __syncthreads();
      if (valid) {   // (integer adds modulo 2^64: the order does not matter)
#pragma unroll
        for (int k = 0; k < 6; k++) atomicAdd(&macc[wid][k][leader], ms[k]);
#pragma unroll
        for (int a = 0; a < 3; a++)
          atomicAdd(&macc[wid][6 + a][leader], (unsigned long long)((long long)w[a] * (1ll << DM_VBITS) + (long long)q[a]));
      }
      __syncthreads();
      if (owner) {
#pragma unroll
        for (int k = 0; k < 6; k++) ms[k] = macc[wid][k][lane];
#pragma unroll
        for (int a = 0; a < 3; a++) {
          const unsigned long long pk = macc[wid][6 + a][lane];
          q[a] = (uint32_t)(pk & ((1ull << DM_VBITS) - 1ull));
          ms[6 + a] = (unsigned long long)((long long)pk >> DM_VBITS);   // (arithmetic shift: floor, and the low field is >= 0)
        }
      }
    } else {
      __shared__ uint32_t acc[4][64][3];
      if (owner) { acc[wid][lane][0] = 0u; acc[wid][lane][1] = 0u; acc[wid][lane][2] = 0u; }
      __syncthreads();
      if (valid) {   // (integer adds: the order does not matter; <= 64 x 2^20 fits 32 bits)
        atomicAdd(&acc[wid][leader][0], q[0]);
        atomicAdd(&acc[wid][leader][1], q[1]);
        atomicAdd(&acc[wid][leader][2], q[2]);
      }
      __syncthreads();
      if (owner) { q[0] = acc[wid][lane][0]; q[1] = acc[wid][lane][1]; q[2] = acc[wid][lane][2]; }
    }
  }
  uint32_t slot = 0;
  bool won = false, ok = true;
  if (owner) ok = dm_find_or_claim(keys, mask, shift, key, slot, won);
  dm_wave_count(&ctr[0], won);
  if (owner && !ok) ctr[3] = 1ull;
  if (owner && ok) {
    unsigned long long* v = vals + 4ull * slot;
    atomicAdd(&v[0], (unsigned long long)cnt);
    atomicAdd(&v[1], (unsigned long long)q[0]);
    atomicAdd(&v[2], (unsigned long long)q[1]);
    atomicAdd(&v[3], (unsigned long long)q[2]);
    if (STAMP) __hip_atomic_store(&aux[2ull * slot + 1], seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (MOMENTS) {
      unsigned long long* mm = mom + (unsigned long long)DM_MOM_WORDS * slot;
#pragma unroll
      for (int k = 0; k < DM_MOM_WORDS; k++) atomicAdd(&mm[k], ms[k]);   // (results unused: no-return atomics)
    }
  }
