// ipk_lab_slots.inc -- the Lab table stage of NS ratios per lane and its out-of-table patch (XYZ_LAB_TRANSFORM.lookup, color_conversions.rs:102-124).
// Included as TEXT, inside a scope, by pointwise4_fast and by the selftest kernel that proves it on every f32 bit pattern (k_selftest_lab_slot), so that both
// compile the very same statements; as a function taking the arrays by reference it gave about 70 guarded kernels 8 to 28 bytes more scratch although their
// statements were the same (profiles/r09_lab_ladder.txt section 2 has the resource figures of every form tried: check them again after a compiler change).
// The including scope provides: constexpr int NS; constexpr bool PXG; const LT *s_lab (LDS); const float v[NS] (the ratios); float f[NS] (the results,
// written here); const int cm (as in pointwise4_fast).
  // The lean body (below) only where there are no per-pixel guards: with the guards' registers live as well its second copy of the slots spills, 12 to 28
  // bytes of scratch in every guarded instantiation (as the masked linear branch does, see the general ladder).
  constexpr bool LAB_LEAN = IPK_LAB_LEAN != 0 && !PXG;
  {
    float pos[NS]; LutPair e[NS];
    #pragma unroll
    for (int k = 0; k < NS; ++k) pos[k] = v[k] * kLutMaxF;
    #pragma unroll
    for (int k = 0; k < NS; ++k) e[k] = lut_pair_at(s_lab, f32_as_u32_sat(pos[k]));
    #pragma unroll
    for (int k = 0; k < NS; ++k) f[k] = e[k].x + __builtin_amdgcn_fractf(pos[k]) * e[k].y;
  }
  bool general = true;
  // (What rounds 1-3 tried around this loop and measured -- LDS queues, one test in front of the twelve, one wait per table stage, slot pairs -- is in profiles/README.md, "The Lab ladder".)
  // One slot = one table-stage value of all 64 lanes.  The wave-row is classified ONCE: as unsigned integers every ratio >= 2, +inf, every NaN, -0 and every negative
  // value is at least 0x40000000 (the bits of 2.0f), so a row whose unsigned maximum over all slots stays below that holds only ratios in [+0, 2) -- an ORDINARY row.
  // Its slots need one compare and one masked region each: `hi` is v > 1, the argument lies in (1, 2) where the short cube root is proven on every f32, and no
  // lane is negative, -0 or NaN.  Every other row takes the general ladder below.  (ipk_selftest_cbrtf variants 3 and 4 run exactly this on every f32 bit pattern.)
  // The two bodies are two `if`s in a row, not if / else: with both on one diamond hipcc keeps a second copy of all NS results alive across the general
  // ladder (+3 VGPRs in every instantiation).  The second test reads the maximum through an empty asm so that the two are not merged again; it costs one
  // compare and one scalar branch per wave-row.
  if (LAB_LEAN) {
    uint32_t vb[NS];
    #pragma unroll
    for (int k = 0; k < NS; ++k) vb[k] = __float_as_uint(v[k]);
    uint32_t vmax = umax_tree<NS>(vb);
    // a row with nothing above the bits of 1.0f stays in the table altogether: one test instead of NS
    general = false;
    if (__builtin_amdgcn_ballot_w64(vmax > 0x3F800000u) != 0) {
      const bool ordinary = __builtin_amdgcn_ballot_w64(vmax >= 0x40000000u) == 0;
      asm("" : "+v"(vmax));
      if (__builtin_expect(__builtin_amdgcn_ballot_w64(vmax >= 0x40000000u) == 0, 1)) {
        // the cube root under the lanes' own mask (see below: what the idle lanes do not burn comes back as clock), written straight into f[k].  The lane test
        // is marked likely so that the body stays in line behind its s_cbranch_execz: left to itself hipcc moves every second body out of line.
        #pragma unroll
        for (int k = 0; k < NS; ++k) { if (__builtin_expect(v[k] > 1.0f, 1)) f[k] = cbrtf_glibc_1to2(v[k]); }
      }
      general = IPK_RARE(!ordinary);
    }
  }
  if (general) {
  // The general ladder.  Per slot that stays in the table this costs a compare and a branch; a slot with lanes above
  // 1 adds one compare, the cube root and one select, and the negative / NaN lanes (their own compare: as a bit pattern they are exactly the
  // values above +inf's) the linear branch.  (Round 2 derived the third mask from the first two -- hipcc moves such a mask through a VGPR to
  // branch on it -- and copied each mask into vcc: 36 instructions per entered slot, 27 now.)
  #pragma unroll
  for (int k = 0; k < NS; ++k) {
    if (IPK_RARE(__builtin_amdgcn_ballot_w64(__float_as_uint(v[k]) > 0x3F800000u) != 0)) {   // some lane has v > 1, v < 0, -0 or NaN
      const bool hi = v[k] > 1.0f;
      // the cube root under the lanes' own mask: the same instructions are issued, but only the lanes above 1 -- a tenth to a third of them on
      // the noise frame -- switch the f64 data path.  The kernel is bound by the socket's power cap, so what the idle lanes do not burn comes back as clock.
      // In the common-parameter variants (cm != 0); the linear branch for negative ratios below is masked only where there are no per-pixel
      // guards (PXG == false): with the guards' registers live as well BOTH masked regions spill (X-Trans full resolution 0.295 -> 0.338 ms with 36
      // bytes of scratch), the cube root's alone does not (X-Trans noise 0.305 -> 0.288 ms).
      if (cm != 0) { if (__builtin_amdgcn_ballot_w64(hi) != 0) { if (hi) f[k] = lab_cbrt(v[k], true); } }
      else if (__builtin_amdgcn_ballot_w64(hi) != 0) { const float c = lab_cbrt(v[k], hi); f[k] = hi ? c : f[k]; }
      const bool lo = __float_as_uint(v[k]) > 0x7F800000u;            // negative (or -0), or NaN: out of the table and not above 1
      if (!PXG && cm != 0) { if (__builtin_amdgcn_ballot_w64(lo) != 0) { if (lo) { const float dv = kLabK * v[k] + 16.0f; f[k] = __builtin_fmaf(dv, rc_hi(116.0f), dv * rc_lo(116.0f)); } } }
      else if (__builtin_amdgcn_ballot_w64(lo) != 0)
      { const float dv = kLabK * v[k] + 16.0f; const float t = __builtin_fmaf(dv, rc_hi(116.0f), dv * rc_lo(116.0f)); f[k] = lo ? t : f[k]; }
    }
  }
  }
