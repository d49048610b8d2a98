// Mover waves of the SP wave-specialised 3x3 kernel (textually included into the `if (mover) { ... }` branch of
// tapconv_sp_kernel, conv_mfma_sp.hip; a one-consumer-per-SIMD variant of round 2 (removed; git history)
// shared it).  The including kernel
// defines SP_NCONS (consumer waves per block: the movers are waves SP_NCONS .. SP_NCONS + 3) and SP_MOVER_PRIO (their
// instruction priority) and provides the kernel-scope names used here (d, g, geometry constants, the LDS images sWin / sW,
// the counters sCR / sCL / sWL / sWR, the epilogue slots sEpi, item_of, SP_STAMP ...).
    // ===================== movers =====================
    // Everything goes global -> REGISTERS -> LDS.  Measured on this kernel: one wave sustains about one 1 KB LDS-DMA
    // instruction per 300 cycles (each seems to wait for the previous one to land), 3.4 bytes per cycle and wave, whatever
    // else the CU or the chip is doing, so four movers cannot bring in the 113 KB a step needs (41 KB window + 72 KB
    // weights) next to 6.9 k cycles of MFMA.  Plain global loads issue ~3x faster and need no LDS slot while in flight:
    // the operands of step k+1 are prefetched into the movers' registers a whole step ahead and written into the window
    // buffer / a weight ring slot the moment the consumers have released it (~100 cycles instead of a memory round trip).
    // Protocol (step k = one K-chunk of one patch; window buffer k & 1; weight ring slot j = kernel column j), mover M(k)
    // fills step k:   loads: column 0, window, column 1 (in the order the stores need them; column 2 follows the store
    //                 of column 0 into the same registers)
    //                 wait CR0 (every consumer holds column 0 of step k-1 in registers) -> store column 0 -> CL0
    //                 wait WR[k&1] (the consumers left the buffer in step k-2)           -> store window   -> WL[k&1]
    //                 wait CR1 -> store column 1 -> CL1;  wait CR2 -> store column 2 -> CL2
    //   consumer(k):  wait WL[k&1], CL0 -> read column 0 -> CR0 -> MFMA | wait CL1 -> read -> CR1 -> MFMA | wait CL2 ->
    //                 read -> CR2 -> MFMA -> WR[k&1] -> epilogue of the item
    // Every wait is for an event whose own prerequisites lie strictly earlier in this order: no cycle.  Counters are
    // bumped with release semantics after the ds_writes have completed (lgkmcnt(0)).
    const int pw = wid - SP_NCONS;
    // The movers issue few instructions, each of which gates thousands of MFMA cycles: top priority on their SIMDs (they
    // are the youngest waves there and would otherwise only get the issue slots the two MFMA streams leave over).
    __builtin_amdgcn_s_setprio(SP_MOVER_PRIO);
    const char* wg = reinterpret_cast<const char*>(d.w);
    const size_t w_chunk = (size_t)9 * 4 * wcout * 16;
    const size_t w_gimage = DUAL ? 2 * (size_t)g.w_gimage : (size_t)g.w_gimage;  // (the geometry was sized for d.Cout channels)
    const char* zero = reinterpret_cast<const char*>(d.zero_line) + (lane & 15) * 16;
    // this lane's role inside a window piece (8 pixels x 128 bytes): lanes 8*px .. 8*px + 7 fetch the 8 operand slots of
    // pixel px = ONE 128-byte line (coalesced), rotated by px: LDS slot s of the pixel holds operand slot (s - px) & 7
    const int l_px = lane >> 3, l_c = ((lane & 7) - l_px) & 7, l_img = l_c >> 2, l_kg = l_c & 3;
    const int half1 = drs_sp_group_bytes(d.in_cs), half2 = HAS2 ? drs_sp_group_bytes(d.in2_cs) : 0;
    const int l_off1 = l_img * half1 + l_kg * 16, l_off2 = l_img * half2 + l_kg * 16;
    constexpr int NPW = (NBLK + 3) / 4;  // window pieces per mover wave (at most): blocks pw + 4*i
    static_assert(NBLK == 4 * (NPW - 1) + 1, "piece distribution: the last round holds block NBLK - 1 only, owned by mover 0");
    // per-lane byte offsets of this wave's window pixels relative to the window origin, computed ONCE (32 bits: a tensor
    // spans less than 2 GB): the per-step work of the fast path is one scalar base pointer + one load per piece
    int off1[NPW];
#pragma unroll
    for (int i = 0; i < NPW; ++i) {
      const int p = (pw + 4 * i) * 8 + l_px;
      const int py = (p * 3641) >> 16, px = p - py * IW;  // p / 18 (exact for p < 1024)
      off1[i] = ((py * d.W + px) * d.in_cs) * 4 + l_off1;
    }
    const bool tail_ok = (NBLK - 1) * 8 + l_px < G::NPIX;  // the last block is half empty
    constexpr int WPC = BNB == 64 ? 6 : 3;  // weight pieces (1 KB) per mover wave and kernel column
    u32x4 wr[2][WPC], ww[NPW];  // column registers: column 2 re-uses column 0's once that one is stored
    // weight piece i of column col: source address and LDS destination of this lane's 16 bytes
    // Address of a weight piece = scalar base of the step (chunk, channel group) + scalar offset of the piece (operand
    // image, kernel row / column, k-group: 32 bits) + this lane's constant byte offset: no per-lane 64-bit arithmetic
    // inside the step loop.
    const unsigned lane_w = BNB == 64 ? (unsigned)lane * 16u : (unsigned)(((lane >> 5) * d.Cout + (lane & 31)) * 16);
    auto piece = [&](int col, bool second, int cc, int n0_, int i, const char*& src, char*& dst) __attribute__((always_inline)) {
      int im, ky, kq;  // operand image, kernel row, (first) k-group of the piece: wave-uniform
      if constexpr (BNB == 64) {  // piece = one (image, ky, k-group) row of 64 channels; second input: (image, k-group)
        const int idx = pw * (second ? 2 : WPC) + i;
        im = second ? idx >> 2 : idx / 12; ky = second ? 0 : (idx % 12) >> 2; kq = idx & 3;
      } else {  // piece = two consecutive k-group rows of 32 channels
        const int row0 = (pw * (second ? 1 : WPC) + i) * 2;
        im = second ? row0 >> 2 : row0 / 12; ky = second ? 0 : (row0 % 12) >> 2; kq = row0 & 3;
      }
      const char* base = second ? reinterpret_cast<const char*>(d.w2) + (size_t)cc * 4 * wcout * 16 + (size_t)n0_ * 16
                                : wg + (size_t)cc * w_chunk + (size_t)n0_ * 16;
      const unsigned soff = second ? (unsigned)im * (unsigned)g.w2_gimage + (unsigned)(kq * wcout * 16)
                                   : (unsigned)im * (unsigned)w_gimage + (unsigned)(((ky * 3 + col) * 4 + kq) * wcout * 16);
      src = base + soff + lane_w;
      dst = sW + im * W_IMAGE + (((second ? 0 : col) * 3 + ky) * 4 + kq) * BNB * 16 + lane * 16;
    };
    const int nwin = pw == 0 ? NPW : NPW - 1;  // window pieces of this wave
    int ring_n0 = -1;  // channel group whose (single) weight chunk the ring holds
    bool prev_fill = false;  // the previous step stored weight columns 1 / 2 into the ring (see the polls behind the window store)
    for (int k = 0; k < S; ++k) {
      if (++c == nck) c = 0;
      if (c == 0) item_of(++ord, n, ty0, tx0, n0);
      // A layer with ONE K-chunk (Cin <= 32) re-uses the same 3 weight columns for every item of a channel group: the ring
      // already holds them, so only the counters advance (72 of the 113 KB a step moves are weights).
      const bool ring_hit = nck == 1 && n0 == ring_n0;
      ring_n0 = n0;
      bool second;
      int cc;
      step_kind(c, second, cc);  // (one-tap steps of the second input interleaved with the 3x3 steps: see the kernel)
      // pieces per column (the second input has one tap: column 0 only)
      int np[3];
#pragma unroll
      for (int col = 0; col < 3; ++col) {
        np[col] = second ? (col == 0 ? (BNB == 64 ? 2 : 1) : 0) : WPC;
        if (ring_hit) np[col] = 0;
      }
      auto load_col = [&](int col) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < WPC; ++i)
          if (i < np[col]) {
            const char* src; char* dst;
            piece(col, second, cc, n0, i, src, dst);
            wr[col & 1][i] = *reinterpret_cast<const u32x4*>(src);
          }
      };
      auto store_col = [&](int col) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < WPC; ++i)
          if (i < np[col]) {
            const char* src; char* dst;
            piece(col, second, cc, n0, i, src, dst);
            *reinterpret_cast<u32x4*>(dst) = wr[col & 1][i];
          }
        sp_wait_lds();
        if (lane == 0) sp_bump(sCL + col);
      };
      SP_STAMP(7);
      // epilogue constants of a new item (one mover wave; issued before every other load of the step: the oldest)
      const bool epi_step = c == 0 && pw == 3;  // (mover 0 carries one window piece more than the others)
      u32x4 ev = {0u, 0u, 0u, 0u};
      if (epi_step) {
        const float* src = nullptr;
        const float* src2 = nullptr;
        if constexpr (FUSE) {
          const int fd1 = d.fuse_dim - 1;
          if (lane < 8) src = d.bias ? d.bias + n0 + lane * 4 : nullptr;
          else if (lane < 40) src = d.fuse_w + (size_t)min((lane - 8) >> 3, fd1) * d.Cout + n0 + ((lane - 8) & 7) * 4;
          else if (lane < 44) ev[0] = __float_as_uint(d.fuse_b[min(lane - 40, fd1)]);
        } else {
          const int which = lane / (EC / 4), o = (lane % (EC / 4)) * 4;
          if (which == 0) { src = d.bias ? d.bias + n0 + o : nullptr; src2 = (HAS2 && d.bias2) ? d.bias2 + n0 + o : nullptr; }
          else if (which == 1) src = (d.post_add && o < d.Cout) ? d.post_add + (size_t)n * d.post_cs + n0 + o : nullptr;
          else if (which == 2) src = (d.out2 && !DUAL) ? d.post2 + (size_t)n * d.post2_cs + n0 + o : nullptr;
        }
        if (src) {
          const float4 a = *reinterpret_cast<const float4*>(src);
          float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
          if (src2) b = *reinterpret_cast<const float4*>(src2);
          ev = u32x4{__float_as_uint(a.x + b.x), __float_as_uint(a.y + b.y), __float_as_uint(a.z + b.z), __float_as_uint(a.w + b.w)};
        }
      }
      load_col(0);
      // ---- window loads ----
      if (!second && ty0 >= 1 && ty0 + TH + 1 <= d.H && tx0 >= 1 && tx0 + TW + 1 <= d.W && cc * KC + KC <= d.Cin) {
        // fast path: every window pixel inside the image, every k-group inside the channel count
        const char* base = reinterpret_cast<const char*>(d.in) +
                           ((((long long)n * d.H + (ty0 - 1)) * d.W + (tx0 - 1)) * d.in_cs + d.in_co) * 4 + cc * 128;
#pragma unroll
        for (int i = 0; i < NPW - 1; ++i) ww[i] = *reinterpret_cast<const u32x4*>(base + (unsigned)off1[i]);
        if (pw == 0) ww[NPW - 1] = *reinterpret_cast<const u32x4*>(tail_ok ? base + (unsigned)off1[NPW - 1] : zero);
      } else if (HAS2 && second && ty0 + TH <= d.H2 && tx0 + TW <= d.W2 && cc * KC + KC <= d.Cin2) {
        // second input (the block's 1x1 shortcut: one tap, window origin = patch origin, no halo), patch inside the image,
        // full K-chunk: scalar base + a 32-bit lane offset per piece.  The consumers of a one-tap step read the 16 x 16 patch
        // pixels only, so a lane whose window pixel lies outside the patch may fetch anything: it takes the patch's first
        // pixel.  Before round 4 every one-tap step went through the per-lane 64-bit address chain of the general path
        // below - ~400 cycles per piece, 11 pieces - with nothing to hide it behind: 0.6 us of MFMAs, 3 - 3.7 us per step.
        const char* base = reinterpret_cast<const char*>(d.in2) +
                           ((((long long)n * d.H2 + ty0) * d.W2 + tx0) * d.in2_cs + d.in2_co) * 4 + cc * 128;
        int lpx = l_px;  // opaque: everything derived from it is loop-invariant, and hoisted out of the step loop it would
        asm volatile("" : "+v"(lpx));  // occupy two dozen registers of a kernel that has none to spare
#pragma unroll
        for (int i = 0; i < NPW; ++i)
          if (i < nwin) {
            const int p = (pw + 4 * i) * 8 + lpx;
            const int py = (p * 3641) >> 16, px = p - py * IW;
            const unsigned o = (py < TH && px < TW) ? (unsigned)(((py * d.W2 + px) * d.in2_cs) * 4 + l_off2) : (unsigned)l_off2;
            ww[i] = *reinterpret_cast<const u32x4*>(base + o);
          }
      } else if (!second && cc * KC + KC <= d.Cin) {
        // border patch, full K-chunk: the window offsets of the fast path hold for every pixel inside the image; the others
        // read the zero line.  (One validity bit per piece, recomputed per step from the item's coordinates: a dozen 32-bit
        // operations per piece instead of the 64-bit address chain of the general path.)
        const char* base = reinterpret_cast<const char*>(d.in) +
                           ((((long long)n * d.H + (ty0 - 1)) * d.W + (tx0 - 1)) * d.in_cs + d.in_co) * 4 + cc * 128;
        int lpx = l_px;  // (opaque, as above)
        asm volatile("" : "+v"(lpx));
#pragma unroll
        for (int i = 0; i < NPW; ++i)
          if (i < nwin) {
            const int p = (pw + 4 * i) * 8 + lpx;
            const int py = (p * 3641) >> 16, px = p - py * IW;
            const int iy = ty0 - 1 + py, ix = tx0 - 1 + px;
            const bool ok = p < G::NPIX && (unsigned)iy < (unsigned)d.H && (unsigned)ix < (unsigned)d.W;
            ww[i] = *reinterpret_cast<const u32x4*>(ok ? base + (unsigned)off1[i] : zero);
          }
      } else {
        // partial K-chunks, a second input whose patch crosses the image border: per-lane validity; anything invalid reads the zero line
        const bool ch_ok = cc * KC + l_kg * 8 < (second ? d.Cin2 : d.Cin);
        int lpx = l_px;  // (opaque, as above)
        asm volatile("" : "+v"(lpx));
#pragma unroll
        for (int i = 0; i < NPW; ++i)
          if (i < nwin) {
            const int p = (pw + 4 * i) * 8 + lpx;
            const int py = (p * 3641) >> 16, px = p - py * IW;
            const char* src;
            bool ok;
            if (!second) {
              const int iy = ty0 - 1 + py, ix = tx0 - 1 + px;
              ok = ch_ok && p < G::NPIX && iy >= 0 && iy < d.H && ix >= 0 && ix < d.W;
              src = reinterpret_cast<const char*>(d.in) +
                    ((((long long)n * d.H + iy) * d.W + ix) * d.in_cs + d.in_co) * 4 + cc * 128 + l_off1;
            } else {
              const int iy = ty0 + py, ix = tx0 + px;
              ok = ch_ok && py < TH && px < TW && iy < d.H2 && ix < d.W2;
              src = reinterpret_cast<const char*>(d.in2) +
                    ((((long long)n * d.H2 + iy) * d.W2 + ix) * d.in2_cs + d.in2_co) * 4 + cc * 128 + l_off2;
            }
            ww[i] = *reinterpret_cast<const u32x4*>(ok ? src : zero);
          }
      }
      load_col(1);
      SP_STAMP(0);
      // ---- stores, each as soon as its destination is free and its loads have landed (in-order vector-memory counter) ----
      if (k >= 1) sp_poll(sCR, (unsigned)SP_NCONS * (unsigned)k, d.fault);
      SP_STAMP(1);
      sp_wait_vm(nwin + np[1]);
      if (epi_step) {  // (every consumer is past the epilogue of the item that used this slot: it holds column 0 of step k - 1)
        float* slot = sEpi + (ord & 1) * (G::EPI / 4);
        if (FUSE && lane >= 40) {
          if (lane < 44) slot[160 + lane - 40] = __uint_as_float(ev[0]);
        } else if (lane < 3 * (EC / 4) || FUSE) {
          if (!FUSE || lane < 40) *reinterpret_cast<u32x4*>(slot + lane * 4) = ev;
        }
      }
      store_col(0);
      load_col(2);  // into column 0's registers; needed two thirds of a step from now
      SP_STAMP(2);
      if (k >= 2) sp_poll(sWR + (k & 1), (unsigned)SP_NCONS * (unsigned)(k >> 1), d.fault);
      sp_wait_vm(np[1] + np[2]);
      {
        char* buf = sWin + (k & 1) * WBUF + lane * 16;
#pragma unroll
        for (int i = 0; i < NPW; ++i)
          if (i < nwin) *reinterpret_cast<u32x4*>(buf + (pw + 4 * i) * 1024) = ww[i];
        sp_wait_lds();
        if (lane == 0) sp_bump(sWL + (k & 1));
      }
      SP_STAMP(3);
      // A step with nothing to put into columns 1 and 2 (a one-tap step, a ring hit) does not wait for the consumers to give
      // those slots up: it only advances their "landed" counters (the mover's own program order keeps them monotonic per
      // step), so its successor's loads are issued a whole step earlier.
      // EXCEPT right behind a step that filled the ring: the landed counters count BUMPS, not movers.  A fast mover that
      // bumped column 1 in the fill step k - 1 and bumps it again here, unconditionally, lifts the counter towards the fill
      // step's threshold on behalf of a slower mover whose column-1 store of step k - 1 has not happened yet - two fast
      // movers are enough for the consumers of step k - 1 to read half-filled slots (found as a bit-level difference in one of
      // ~50 k forwards: the first item of a block of conv_blocks.1.conv1, the one launch whose items are single ring-hit steps;
      // tools/diag_determinism.py).  Column 0 cannot run ahead (its bump follows the CR poll above).  The poll on the
      // consumers' release of step k - 1 closes it: they pass their landed poll on four genuine bumps only.
      const bool after_fill = prev_fill;
      prev_fill = np[1] != 0 || np[2] != 0;  // (columns 1 / 2 only: one-tap steps in a row have nothing there to protect)
      if (k >= 1 && (np[1] || after_fill)) sp_poll(sCR + 1, (unsigned)SP_NCONS * (unsigned)k, d.fault);
      SP_STAMP(4);
      sp_wait_vm(np[2]);
      store_col(1);
      if (k >= 1 && (np[2] || after_fill)) sp_poll(sCR + 2, (unsigned)SP_NCONS * (unsigned)k, d.fault);
      SP_STAMP(5);
      sp_wait_vm(0);
      store_col(2);
      SP_STAMP(6);
    }
