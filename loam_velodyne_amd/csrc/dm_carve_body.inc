// The body of the carve kernels of densemap.hip, included textually in each (so that both compile from one text and k_dm_carve keeps
// its instruction stream): the rays of one call's n points from the origin of F.  In scope: n, F (DmFilter), R (DmCarve), keys, aux,
// mask, shift, ctr and the macro DM_CARVE_POINT(j), point j of the call as a float4
  const unsigned long long span = 256ull * R.stride, base = (unsigned long long)blockIdx.x * span;
  uint32_t left_out = 0u;
  if (R.stride > 1u) {
    const unsigned long long end = base + span < (unsigned long long)n ? base + span : (unsigned long long)n;
    for (unsigned long long j = base + threadIdx.x; j < end; j += 256ull) {
      float d2;
      if (j % R.stride != 0ull && dm_added(DM_CARVE_POINT(j), F, d2)) left_out++;
    }
  }
  const unsigned long long i = base + (unsigned long long)threadIdx.x * R.stride;
  bool traced = false, skip_range = false, skip_steps = false, overflow = false;
  uint32_t visited = 0u, missed = 0u;
  if (i < (unsigned long long)n) {
    const float4 p = DM_CARVE_POINT(i);
    float d2;
    if (dm_added(p, F, d2)) {
      if (R.use_max && !(d2 <= R.max2)) {
        skip_range = true;
      } else {
        DmAxis X, Y, Z;
        const bool okx = dm_axis_setup(F.ox, p.x, F.inv, X), oky = dm_axis_setup(F.oy, p.y, F.inv, Y), okz = dm_axis_setup(F.oz, p.z, F.inv, Z);
        const uint32_t n_steps = X.rem + Y.rem + Z.rem;   // (each < 2^21)
        if (!(okx && oky && okz) || n_steps > R.max_steps) {
          skip_steps = true;
        } else {
          traced = true;
          // cells k = 0 .. n_steps - 1 - end_margin are visited; cell k is the cell after k steps
          const uint32_t n_visit = n_steps > R.end_margin ? n_steps - R.end_margin : 0u;
          for (uint32_t k = 0; k < n_visit; k++) {
            uint32_t slot = 0u;
            const int f = dm_find(keys, mask, shift, dm_key(X.c, Y.c, Z.c), slot);
            visited++;
            if (f < 0) overflow = true;
            if (f > 0 && aux[2ull * slot + 1] != R.seq) {   // occupied wins: a voxel this call hit is left alone
              atomicAdd(&aux[2ull * slot], 1u);
              missed++;
            }
            dm_walk_step(X, Y, Z);   // (k < n_steps: some axis has cells left)
          }
        }
      }
    }
  }
  if (overflow) ctr[3] = 1ull;
  dm_wave_count(&ctr[4], traced);
  dm_wave_sum(&ctr[5], left_out);
  dm_wave_count(&ctr[6], skip_range);
  dm_wave_count(&ctr[7], skip_steps);
  dm_wave_sum(&ctr[8], visited);
  dm_wave_sum(&ctr[9], missed);
