// The body of the pair-tile kernels (ppk_dist.hip): dist_kernel_v2, dist_kernel_v2_rank and dist_kernel_v2_fold2 include
// it between their braces.  It is text, not a function, on purpose: the kernels sit at the register limit, and the same body
// inlined from a __device__ function compiles to other code (the by-value DistParams is then read differently).
// In scope at the point of inclusion: the kernel's arguments (refT, qryT, lut, ref_clu, qry_clu, rtab, out, n_failed,
// mask_out, p) and the compile-time constants NW, MODE, W, KSPLIT, WIDE, EXP, FOLD2 (the two-holder pair: one block at the
// top of the epilogue), FOLDH (with FOLD2: the holder pair -- 4 / 3 / 2-plane streams and 12-bit corrections) and
//   PL: the bit-planes a 64-bin block is copied and compared in.  14 = the sketch's own bbits; 8, 10 or 12 on a
//       rank-coded database (ppk_db::d_skR: every bin value replaced by its rank among the distinct values of its
//       (k, bin) position, which keeps "equal / not equal" and so every count).  The collision adjustment and the fit
//       table still see the real width (V2_BB).  A block whose flag in DistParams::rank_short is set ("short": every
//       code of the block is below 2^(PL-1), plane PL-1 is zero) is copied whole and compared in PL - 1 planes.
  static_assert(NW == 8, "the product tile is 256 refs x 32 queries (8 wavefronts)");
  static_assert(PL == V2_BB || (PL >= 8 && PL < V2_BB && PL % 2 == 0 && W == 2 && !KSPLIT && !WIDE && !EXP &&
                                (MODE == MODE_DIST || ppk_is_mask(MODE))),
                "rank-coded planes: the two-dword whole-tile kernel only");
  // WIDE without KSPLIT: the tile kernel whose count register windows the k list (PackWide).  WIDE with KSPLIT: a
  // k-split unit (it counts ONE k, or a piece of one: W = 2 holds it) whose tile is fitted by its last unit straight
  // from the units' partial counts (PackParts) -- no count register is ever rebuilt, so any k list fits.
  static_assert(!WIDE || (KSPLIT ? (W == 2 && (MODE == MODE_DIST || ppk_is_mask(MODE)))
                                 : (W == 4 && (MODE == MODE_DIST || ppk_is_mask(MODE) || MODE == MODE_KNN))),
                "the wide instantiations");
  constexpr bool WIDE_TILE = WIDE && !KSPLIT;
  const int ablate = EXP ? p.ablate : 0;
  constexpr int R = V2_R, TQ = V2_TQ, BB = V2_BB;
  constexpr int V2_QT = NW * TQ;              // queries per workgroup tile (32)
  // CPL: the planes of a STORED chunk, which is what is copied.  PL everywhere but on the holder pair, whose blocks
  // never span more than 16 codes: its copies keep planes 0 .. 3 only (PPK_FOLDH_CHUNK_PLANES), 8 ref pieces and one
  // query piece per block, two DMA pieces per wavefront
  constexpr int CPL = FOLDH ? PPK_FOLDH_CHUNK_PLANES : PL;
  constexpr int REF_U4 = CPL * 128;           // 14 rows x 256 samples x 8 B = 28 KB
  constexpr int QRY_U4 = CPL * (V2_QT / 2);   // 14 rows x QT samples x 8 B = 3.5 / 7 KB
  constexpr int CHUNK_U4 = REF_U4 + QRY_U4;   // one 64-bin block of the tile
  constexpr int LPP = V2_QT / 2;              // lanes (16 B each) per query row
  constexpr int PPP = 64 / LPP;               // query rows per one-KB DMA piece
  constexpr int NQP = (CPL + PPP - 1) / PPP;  // query pieces per chunk
  constexpr int NPIECE = 2 * CPL + NQP;       // 28 ref pieces + query pieces
  constexpr int PW = (NPIECE + NW - 1) / NW;  // DMA pieces per wavefront per chunk
  // double buffer: 63 KB.  The modes with a per-pair fit take 80 KB -- two workgroups then own all
  // 160 KB of a CU -- so that the epilogue of an interior tile can hold the whole (E, F) table
  // (5 k x 1024 counts x 16 B) in LDS, see below.
  constexpr bool LDS_TABLE = NW == 8 && W == 2 && !WIDE && (MODE == MODE_DIST || ppk_is_mask(MODE) || MODE == MODE_KNN);
  constexpr int TAB_U4 = 5 * 1024;
  // KS_FUSED: a k-split job whose tiles are fitted by their last workgroup (below); one more entry behind the
  // compare buffers holds the workgroup's grid position across the loop, in LDS instead of two SGPRs
  constexpr bool KS_FUSED = KSPLIT && (MODE == MODE_DIST || ppk_is_mask(MODE));
  constexpr bool KS_MEM = KS_FUSED && WIDE;
  constexpr int KS_SLOT = 2 * CHUNK_U4;      // (WIDE: the workgroup's spill slot index lives there)
  __shared__ u32x4 lds[LDS_TABLE && TAB_U4 > 2 * CHUNK_U4 + 1 ? TAB_U4 : 2 * CHUNK_U4 + (KS_FUSED || WIDE ? 1 : 0)];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // Tile order.  Workgroup b runs on XCD b % 8 (observed dispatch order; used for speed only).
  // Each XCD has a private 4 MB L2, so XCD x is given the ref tiles rt = x, x+8, ... and walks
  // the query tiles with its few ref tiles innermost: the ~64 workgroups resident on an XCD then
  // share the same ref rows through that L2 instead of every XCD streaming every ref tile.
  size_t rt, qt;
  const bool strip = blockIdx.x < p.n_strip;      // workgroup-uniform
  // the band of query rows this tile filters on, and where its query tiles start
  size_t qb = p.q_begin, qe = p.q_end, q_tile0 = p.q_tile0;
  if (strip) {
    // strip tiles come first in the grid so that their serial latency overlaps everything else
    rt = p.strip_rt0 + blockIdx.x % p.strip_r_tiles;
    qt = blockIdx.x / p.strip_r_tiles;
    qb = p.strip_begin;
    qe = p.n_ref;
    q_tile0 = p.strip_begin / V2_QT;
  } else {
    if (blockIdx.x < p.n_strip_pad) return;
    const unsigned b = blockIdx.x - p.n_strip_pad;
    if (!EXP || p.xcd_map == 0) {
      // Default order.  Workgroup b is dispatched to XCD b % (number of XCDs) (observed, tools/ubench_grid_xcd.hip;
      // used for speed only) and every XCD has a private 4 MB L2.  The non-empty tiles, taken ref-tile-major, are
      // cut into as many equal contiguous runs as the device has XCDs (ppk_geometry: 8 on MI355X), one per XCD: the ~64 workgroups resident on an XCD then work on
      // one or two ref tiles at a time (their rows are fetched into that L2 once per 64-bin block
      // and re-used by all of them), and the XCDs are balanced to one tile whatever the shape of
      // the job (in the triangular self job high ref tiles carry more query tiles than low ones).
      const unsigned x = b & ((1u << p.xcd_shift) - 1u), j = b >> p.xcd_shift;
      const unsigned g = x * p.tiles_per_xcd + j;
      if (j >= p.tiles_per_xcd || g >= p.n_tiles) return;
      unsigned lo = 0, hi = p.r_tiles - 1;      // largest ref tile with tiles_before(rt) <= g
      while (lo < hi) {
        const unsigned mid = (lo + hi + 1) >> 1;
        if (tiles_before(mid, p.self, p.q_tiles, p.tri_m, p.tri_c0) <= g) lo = mid;
        else hi = mid - 1;
      }
      rt = lo;
      qt = g - tiles_before(lo, p.self, p.q_tiles, p.tri_m, p.tri_c0);
    } else if (p.xcd_map == 1) {
      const unsigned xcd = b & 7u, j = b >> 3;
      if (xcd >= p.r_tiles) return;
      const unsigned nloc = (p.r_tiles - xcd + 7u) >> 3;   // ref tiles owned by this XCD
      qt = j / nloc;
      rt = xcd + 8u * (j % nloc);
      if (qt >= p.q_tiles) return;
    } else {
      // (A/B only, PPK_MAP=2)  With rt = b % r_tiles and r_tiles a multiple of 8
      // every ref tile would stay on one XCD, and in the triangular job high ref tiles carry more
      // query tiles than low ones: XCD 7 would get ~40 % more work than XCD 0.  Skewing each
      // query-tile row by its index rotates the ref tiles over the XCDs.
      // (ref x query jobs are balanced as they are, and keeping a ref tile on one XCD lets its
      // rows be re-used from that XCD's L2: measured 3 % faster un-skewed)
      qt = b / p.r_tiles;
      rt = p.self ? (b % p.r_tiles + qt) % p.r_tiles : b % p.r_tiles;
    }
  }
  const size_t r0 = rt * V2_RT;
  const size_t q0 = (q_tile0 + qt) * V2_QT;
  const size_t qw0 = q0 + (size_t)wave * TQ;
  const bool tri = p.self && !strip;              // upper-triangle tile: pairs need r > q
  if (tri && r0 + (V2_RT - 1) <= q0) return;      // no pair with r > q in this tile
  // diagonal tile whose queries all lie beyond the first 128 refs: the lanes' refs 0/1 pair with
  // nothing, so their rows are neither copied nor compared (8-wave shape)
  const bool half = NW == 8 && tri && q0 >= r0 + 128;
  const bool wave_active = !(tri && r0 + (V2_RT - 1) <= qw0) && qw0 < qe && qw0 + TQ > qb;
  // lane l owns refs r0 + {2l, 2l+1, 128+2l, 128+2l+1}: two conflict-free ds_read_b128 per plane
  // (recomputed where needed rather than kept live across the compare loop)
  int lane_late = lane;   // DIST / MASK: re-derived after the loop, see below
  auto ref_of = [&](int r) -> size_t { return r0 + 2 * lane_late + (r & 1) + (r >> 1) * 128; };

  if constexpr (WIDE_TILE) {
    // take a spill slot: the first free bit from a start that spreads neighbouring workgroups over the words
    if (threadIdx.x == 0) {
      const unsigned mask = p.wide_nslots - 1u;
      unsigned sl = (blockIdx.x * 37u) & mask;
      for (;;) {
        const unsigned bit = 1u << (sl & 31u);
        // acquire / release at agent scope around a slot's ownership: the next owner may run on another XCD.  (Once
        // per workgroup, off the compare loop: the two cache operations the pair implies are not felt here.)
        const unsigned old = __hip_atomic_fetch_or(p.wide_bitmap + (sl >> 5), bit, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (!(old & bit)) break;
        sl = (sl + 1u) & mask;
        if ((sl & 31u) == 0) __builtin_amdgcn_s_sleep(8);
      }
      u32x4 pos;
      pos.x = sl;
      pos.y = pos.z = pos.w = 0;
      lds[KS_SLOT] = pos;      // (read after the first barrier below)
    }
  }
  // one chunk per (k, 64-bin block); with k_split a workgroup owns the chunks of k = blockIdx.y only
  // (a template parameter, not a launch parameter: the tile kernels sit at the SGPR limit and one
  // more live scalar spills into VGPR lanes and from there into scratch inside the loop)
  // (KSPLIT: workgroup y owns the ks_blocks consecutive blocks of unit y -- the resident layout is
  // [k][block][plane][sample], so unit y = k * k_split + piece starts at block y * ks_blocks)
  const int k_first = KSPLIT ? (int)blockIdx.y : 0;
  const int ublocks = KSPLIT ? p.ks_blocks : p.s64;       // blocks per k (per unit)
  const int total = KSPLIT ? ublocks : p.nk * p.s64;
  if constexpr (KS_FUSED) {
    if (threadIdx.x == 0) {
      u32x4 pos;
      pos.x = blockIdx.x;
      pos.y = blockIdx.y;
      pos.z = pos.w = 0;
      lds[KS_SLOT] = pos;
    }
  }

  // DMA sources: each wavefront copies PW of the chunk's one-KB pieces (28 ref pieces: row i/2,
  // half i%2; then the query pieces: PPP rows x LPP lanes each).  A piece's address is a
  // wave-uniform base (advanced by one 64-bin block = 14 rows per chunk) plus a per-lane 32-bit
  // byte offset, i.e. the saddr+voffset form of global_load_lds_dwordx4.
  const char *dbase[PW];
  size_t dstep[PW];
  int doff[PW];
  int dkind[PW];   // 0 = ref piece, 1 = query piece, 2 = none
#pragma unroll
  for (int t = 0; t < PW; ++t) {
    const int i = wave + NW * t;
    dbase[t] = nullptr;
    dstep[t] = 0;
    doff[t] = 0;
    if (i < 2 * CPL) {
      dkind[t] = 0;
      dbase[t] = reinterpret_cast<const char *>(refT + ((size_t)k_first * ublocks * CPL + (size_t)(i >> 1)) * p.npad_r + r0 + (i & 1) * 128);
      dstep[t] = (size_t)CPL * p.npad_r * 8;
      doff[t] = i * 64;
    } else if (i < NPIECE) {
      const int j = i - 2 * CPL;
      dkind[t] = 1;
      dbase[t] = reinterpret_cast<const char *>(qryT + ((size_t)k_first * ublocks * CPL + (size_t)(PPP * j)) * p.npad_q + q0);
      dstep[t] = (size_t)CPL * p.npad_q * 8;
      doff[t] = REF_U4 + j * 64;
    } else {
      dkind[t] = 2;
    }
  }
  const uint32_t voff_ref = lane * 16;
  const uint32_t voff_qry = (uint32_t)((lane / LPP) * p.npad_q * 8) + (lane % LPP) * 16;
  // the last query piece may hold fewer than PPP rows (14 and 10 are no multiples of 4)
  const bool qlane_ok = (PPP * (NQP - 1) + lane / LPP) < CPL;
  // skip_first_half: a half tile does not copy the even ref pieces (samples 0..127 of each row);
  // with 8 waves piece parity is wave parity
  auto issue_dma = [&](int buf, bool skip_first_half) {
    u32x4 *base = lds + buf * CHUNK_U4;
#pragma unroll
    for (int t = 0; t < PW; ++t) {
      if (dkind[t] == 0) {
        if (!(skip_first_half && (wave & 1) == 0))
          __builtin_amdgcn_global_load_lds(PPK_GPTR(dbase[t] + voff_ref), PPK_LPTR(base + doff[t]), 16, 0, 0);
      } else if (dkind[t] == 1 && (wave + NW * t != NPIECE - 1 || qlane_ok)) {
        __builtin_amdgcn_global_load_lds(PPK_GPTR(dbase[t] + voff_qry), PPK_LPTR(base + doff[t]), 16, 0, 0);
      }
      dbase[t] += dstep[t];
    }
  };

  using PackT = PackW<W>;
  uint32_t pw[W][R][TQ];      // the count registers, dword-major; pw[0] counts the current k
#pragma unroll
  for (int i = 0; i < W; ++i)
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = 0; q < TQ; ++q) pw[i][r][q] = 0;

  typedef const __attribute__((address_space(4))) DistParams LateParams;
  // WIDE: park the count registers of group g in the workgroup's spill slot (PackWide).  Everything it needs
  // beyond the registers themselves is fetched when it runs -- once per wide_kpg * s64 blocks -- so the loop
  // carries one more scalar (`wide_next`) and nothing else.
  auto wide_park = [&](int g) __attribute__((always_inline)) {
    if constexpr (WIDE_TILE) {
      const char __attribute__((address_space(4))) *ka =
          (const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
      asm volatile("" : "+s"(ka));
      LateParams &pl = *reinterpret_cast<LateParams *>(ka + V2_PARAMS_KERNARG_OFFSET);
      const uint32_t slot = __builtin_amdgcn_readfirstlane(*(volatile __attribute__((address_space(3))) uint32_t *)(__attribute__((address_space(3))) void *)(lds + KS_SLOT));
      // uniform base + one 32-bit lane offset (the saddr form): dword stores, written through (sc1 = agent scope)
      const char *dst = reinterpret_cast<const char *>(pl.wide_slots + ((size_t)slot * (size_t)pl.wide_groups + (size_t)g) * WIDE_GROUP_U64);
      const uint32_t voff = (uint32_t)wave * 256u + (voff_ref >> 2);      // 4 * thread
#pragma unroll
      for (int q = 0; q < TQ; ++q)
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int i = 0; i < W; ++i) {
            // dword i of pair (q, r): [(q * R + r) * 4 + i][512 threads]
            const char *d = dst + (size_t)(((q * R + r) * 4 + i) * 2048);
            asm volatile("global_store_dword %0, %1, %2 sc1" ::"v"(voff), "v"(pw[i][r][q]), "s"(d) : "memory");
          }
    }
  };

  // PL < 14: the "short" flags of the blocks of k `kk`, one bit per block (DistParams::rank_short).  Fetched through the
  // kernarg segment pointer, opaquely, once per k -- where the loop does its end-of-k work -- so that the loop carries
  // one scalar for them and no load or wait stands in front of a block.
  auto rank_short_word = [&](int kk) __attribute__((always_inline)) -> uint32_t {
    const char __attribute__((address_space(4))) *ka =
        (const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    LateParams &pl = *reinterpret_cast<LateParams *>(ka + V2_PARAMS_KERNARG_OFFSET);
    return pl.rank_short[kk];
  };
  // FOLD2: the second flag word of k `kk` (DistParams::fold2_six: the blocks that compare 6 planes), fetched the same way
  auto fold2_six_word = [&](int kk) __attribute__((always_inline)) -> uint32_t {
    const char __attribute__((address_space(4))) *ka =
        (const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    LateParams &pl = *reinterpret_cast<LateParams *>(ka + V2_PARAMS_KERNARG_OFFSET);
    return pl.fold2_six[kk];
  };

  issue_dma(0, half);
  if (!(ablate & 16)) {   // (bit 16, measurement only: what hiding the tile's first copy could win)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  // the whole loop is instantiated twice (full / half block) rather than branching around the two
  // instruction streams inside it: a live `half` flag costs the one register the loop does not have
  auto compare_loop = [&](auto half_tag) {
  constexpr bool HALF = decltype(half_tag)::value;
  int k = k_first, blk = 0;
  // the full block of a rank-coded database leaves the top plane out where the block's flag says it is zero (the half
  // block of the diagonal tiles compares every plane: a zero plane changes no count, and those tiles are few)
  constexpr bool SHORT_BLOCKS = PL < V2_BB && !HALF;
  uint32_t short_w = 0;
  if constexpr (SHORT_BLOCKS) short_w = rank_short_word(k);
  uint32_t six_w = 0;
  if constexpr (SHORT_BLOCKS && FOLD2) six_w = fold2_six_word(k);
  for (int g = 0; g < total; ++g) {
    const int buf = g & 1;
    // the other buffer was last read in iteration g-1, which every wave left through the barrier
    // The packed modes run the variant of the full block that issues the
    // wave's four DMA pieces from INSIDE its instruction stream (in VALU-only stretches instead of
    // next to the opening burst of ds_reads); waves with nothing to compare still copy from here.
    constexpr bool DMA_IN_STREAM = NW == 8 && W >= 2 && !HALF;
    if (g + 1 < total && !(ablate & 4) && !(DMA_IN_STREAM && wave_active)) issue_dma(buf ^ 1, HALF);

    if (wave_active && !(ablate & 2)) {
      // One 64-bin block of the 4x4 register tile: 14 x (4 ds_read_b128 + 32 v_bitop3) + 32
      // v_bcnt, as the generated bank-aware instruction stream (tools/gen_block_asm.py).
      const uint32_t rp =
          (uint32_t)(size_t)(__attribute__((address_space(3))) void *)(lds + buf * CHUNK_U4) + voff_ref;
      const uint32_t qp = (uint32_t)(size_t)(__attribute__((address_space(3))) void *)(
          lds + buf * CHUNK_U4 + REF_U4 + wave * 2);
// The counters are pinned to v56..v71 in the order that keeps every v_bcnt's two VGPR sources (the
// stream's accumulator v96+2j / v97+2j and counter j) in different register banks: left to the
// allocator, 7 of the 32 v_bcnt of a block collided.
#define PPK_BLOCK_OPERANDS                                                                   \
  [c0] "+{v58}"(pw[0][0][0]), [c1] "+{v56}"(pw[0][0][1]), [c2] "+{v59}"(pw[0][0][2]), [c3] "+{v57}"(pw[0][0][3]), \
      [c4] "+{v62}"(pw[0][1][0]), [c5] "+{v60}"(pw[0][1][1]), [c6] "+{v63}"(pw[0][1][2]), [c7] "+{v61}"(pw[0][1][3]), \
      [c8] "+{v66}"(pw[0][2][0]), [c9] "+{v64}"(pw[0][2][1]), [c10] "+{v67}"(pw[0][2][2]), [c11] "+{v65}"(pw[0][2][3]), \
      [c12] "+{v70}"(pw[0][3][0]), [c13] "+{v68}"(pw[0][3][1]), [c14] "+{v71}"(pw[0][3][2]), [c15] "+{v69}"(pw[0][3][3])
// (one asm statement per plane count: the stream is a string literal)
#define PPK_BLOCK_BY_PLANES(STMT)                     \
  if constexpr (PL == 14) { STMT() }                  \
  else if constexpr (PL == 12) { STMT(_P12) }         \
  else if constexpr (PL == 10) { STMT(_P10) }         \
  else { static_assert(PL == 14 || PL == 12 || PL == 10 || PL == 8, "plane counts with a generated stream"); STMT(_P8) }
      if constexpr (NW == 8) {
        if constexpr (HALF) {
#define PPK_HALF_STMT(SUF)                                                                                  \
  asm volatile(PPK_BLOCK_HALF_ASM_Q32##SUF : PPK_BLOCK_OPERANDS : [rp] "v"(rp), [qp] "v"(qp) \
               : "memory", PPK_BLOCK_CLOBBERS);
          if constexpr (FOLDH) {      // (every plane of the holder pair's 4-plane chunk)
            asm volatile(PPK_BLOCK_HALF_H4_ASM_Q32_P4 : PPK_BLOCK_OPERANDS : [rp] "v"(rp), [qp] "v"(qp)
                         : "memory", PPK_BLOCK_CLOBBERS);
          } else {
            PPK_BLOCK_BY_PLANES(PPK_HALF_STMT)
          }
#undef PPK_HALF_STMT
        } else if constexpr (DMA_IN_STREAM) {
          // the in-stream variant issues the wavefront's PW pieces: PW - 1 ref pieces 8 KB apart and a LAST one that is a
          // ref piece, a query piece or (fewer than 8 PW pieces in a block) nothing, by wavefront
          static_assert(NW != 8 || PW == (FOLDH ? 2 : PL >= 12 ? 4 : 3), "DMA pieces per wavefront of the generated stream");
          static_assert(2 * CPL >= NW * (PW - 1), "every piece but a wavefront's last is a ref piece");
          constexpr int LT = PW - 1;
          const uint32_t lbase =
              (uint32_t)(size_t)(__attribute__((address_space(3))) void *)(lds + (buf ^ 1) * CHUNK_U4);
          const uint32_t m00 = __builtin_amdgcn_readfirstlane(lbase + (uint32_t)doff[0] * 16u);
          const uint32_t m03 = __builtin_amdgcn_readfirstlane(lbase + (uint32_t)doff[LT] * 16u);
          // the last piece is a ref piece for the first waves and a query piece for the next ones; the last query
          // piece may hold fewer rows than lanes, and a wave past the last piece copies nothing (exec mask 0)
          constexpr bool LAST_MAY_BE_EMPTY = NW * PW > NPIECE;
          const uint64_t xb = (LAST_MAY_BE_EMPTY && dkind[LT] == 2) ? 0ull : (wave + NW * LT == NPIECE - 1) ? __ballot(qlane_ok) : ~0ull;
          const uint32_t xblo = __builtin_amdgcn_readfirstlane((uint32_t)xb),
                         xbhi = __builtin_amdgcn_readfirstlane((uint32_t)(xb >> 32));
          const uint32_t vob = dkind[LT] == 0 ? voff_ref : voff_qry;
          // PL < 14: the statement holds the full and the short stream and picks one on bit blk of short_w (a scalar
          // bit test and a branch inside the asm: the compiler sees one statement, as in the raw kernel)
#define PPK_DMA_SEL_STMT(SUF, SB2)                                                                                \
  asm volatile(PPK_BLOCK_DMA_SEL_ASM_Q32##SUF                                                                     \
               : PPK_BLOCK_OPERANDS                                                                               \
               : [rp] "v"(rp), [qp] "v"(qp), [m00] "s"(m00), [m03] "s"(m03), [sb0] "s"(dbase[0]),                 \
                 [sb1] "s"(dbase[1]), [sb2] "s"(dbase[SB2]), [sb3] "s"(dbase[LT]), [voa] "v"(voff_ref),           \
                 [vob] "v"(vob), [xblo] "s"(xblo), [xbhi] "s"(xbhi), [sh] "s"(short_w), [bk] "s"(blk)             \
               : "memory", "scc", PPK_BLOCK_CLOBBERS);
          // FOLD2: three streams, 8 / 7 / 6 planes, on bit blk of short_w and of six_w (FOLDH: 4 / 3 / 2 planes, the
          // words then hold DistParams' flags of the holder pair)
#define PPK_DMA_SEL3_STMT(SUF, SB2) PPK_DMA_SEL3_STMT_OF(PPK_BLOCK_DMA_SEL3_ASM_Q32##SUF, SB2)
#define PPK_DMA_SEL3_STMT_OF(STREAM, SB2)                                                                         \
  asm volatile(STREAM                                                                                             \
               : PPK_BLOCK_OPERANDS                                                                               \
               : [rp] "v"(rp), [qp] "v"(qp), [m00] "s"(m00), [m03] "s"(m03), [sb0] "s"(dbase[0]),                 \
                 [sb1] "s"(dbase[1]), [sb2] "s"(dbase[SB2]), [sb3] "s"(dbase[LT]), [voa] "v"(voff_ref),           \
                 [vob] "v"(vob), [xblo] "s"(xblo), [xbhi] "s"(xbhi), [sh] "s"(short_w), [sh2] "s"(six_w),         \
                 [bk] "s"(blk)                                                                                    \
               : "memory", "scc", PPK_BLOCK_CLOBBERS);
          if constexpr (PL < V2_BB) {
            if constexpr (PL == 12) { PPK_DMA_SEL_STMT(_P12, 2) }
            else if constexpr (PL == 10) { PPK_DMA_SEL_STMT(_P10, LT) }
            else if constexpr (FOLDH) { PPK_DMA_SEL3_STMT_OF(PPK_BLOCK_DMA_SELH_ASM_Q32_P4, LT) }
            else if constexpr (FOLD2) { PPK_DMA_SEL3_STMT(_P8, LT) }
            else { PPK_DMA_SEL_STMT(_P8, LT) }
          } else {
            asm volatile(PPK_BLOCK_DMA_ASM_Q32
                         : PPK_BLOCK_OPERANDS
                         : [rp] "v"(rp), [qp] "v"(qp), [m00] "s"(m00), [m03] "s"(m03), [sb0] "s"(dbase[0]),
                           [sb1] "s"(dbase[1]), [sb2] "s"(dbase[2]), [sb3] "s"(dbase[3]), [voa] "v"(voff_ref),
                           [vob] "v"(vob), [xblo] "s"(xblo), [xbhi] "s"(xbhi)
                         : "memory", "scc", PPK_BLOCK_CLOBBERS);
          }
#undef PPK_DMA_SEL_STMT
#undef PPK_DMA_SEL3_STMT
#undef PPK_DMA_SEL3_STMT_OF
          // (after the last block the pieces harmlessly re-load it into the idle buffer)
          if (g + 2 < total) {
#pragma unroll
            for (int t = 0; t < PW; ++t) dbase[t] += dstep[t];
          }
        } else {
          static_assert(PL == V2_BB, "the unpacked modes compare raw planes");
          asm volatile(PPK_BLOCK_ASM_Q32 : PPK_BLOCK_OPERANDS : [rp] "v"(rp), [qp] "v"(qp)
                       : "memory", PPK_BLOCK_CLOBBERS);
        }
      }
#undef PPK_BLOCK_BY_PLANES
#undef PPK_BLOCK_OPERANDS

      if constexpr (KS_FUSED) {
        // one unit = part of one k: nothing happens between blocks, the counts leave after the loop
      } else if (blk == ublocks - 1) {
        // ---- end of one k --------------------------------------------------------
        if constexpr (MODE == MODE_DIST || ppk_is_mask(MODE) || MODE == MODE_KNN) {
          // another k follows: the count register moves up by one field
          bool parked = false;
          if constexpr (WIDE_TILE) {
            // (the group size is fetched here, opaquely: held across the loop it costs the scalar -- and, hoisted,
            // the reciprocal -- the loop does not have; this runs once per s64 blocks)
            int kpg = p.wide_kpg;
            asm volatile("" : "+s"(kpg));
            if (k + 1 < p.nk && (k + 1) % kpg == 0) {
              // the register holds a whole group: out it goes, the next group starts from zero
              wide_park((k + 1) / kpg - 1);
#pragma unroll
              for (int i = 0; i < W; ++i)
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                  for (int q = 0; q < TQ; ++q) pw[i][r][q] = 0;
              parked = true;
            }
          }
          if (k + 1 < p.nk && !parked) {
            const int up = 32 - p.cnt_bits;
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
              for (int q = 0; q < TQ; ++q) {
#pragma unroll
                for (int i = W - 1; i > 0; --i)
                  pw[i][r][q] = __builtin_amdgcn_alignbit(pw[i][r][q], pw[i - 1][r][q], up);
                pw[0][r][q] <<= p.cnt_bits;
              }
          }
        } else {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int q = 0; q < TQ; ++q) {
            {
              const size_t qq = qw0 + q, rf = ref_of(r);
              const bool valid = rf < p.r_limit && qq >= qb && qq < qe && (!p.self || rf > qq);
              if (valid) {
                const size_t row = (p.self ? qq * p.n_ref - (qq * (qq + 1)) / 2 + (rf - qq - 1)
                                           : qq * p.n_ref + rf) - p.row_base;
                if constexpr (MODE == MODE_COUNTS && KSPLIT) {
                  // private k-major layout: consecutive lanes write consecutive rows
                  static_cast<uint32_t *>(out)[(size_t)k * p.ks_rows + row] = pw[0][r][q];
                } else if constexpr (MODE == MODE_COUNTS) {
                  static_cast<uint32_t *>(out)[row * p.nk + k] = pw[0][r][q];
                } else {
                  double jr = 0.0;
                  if (p.random_correct) {
                    const int cr = ref_clu ? ref_clu[rf] : 0;
                    const int cq = qry_clu ? qry_clu[qq] : 0;
                    jr = (double)rtab[((size_t)k * p.n_clu + cr) * p.n_clu + cq];
                  }
                  static_cast<float *>(out)[row * p.nk + k] =
                      (float)observed_excess(jaccard_obs(pw[0][r][q], p.s64, BB, p.ext_adjust), jr);
                }
              }
            }
            pw[0][r][q] = 0;
          }
        }
      }
    }
    if constexpr (!KS_FUSED) {
      if (++blk == ublocks) {
        blk = 0;
        ++k;
        if constexpr (SHORT_BLOCKS) short_w = rank_short_word(k);      // (word nk after the last k: in the array, unused)
        if constexpr (SHORT_BLOCKS && FOLD2) six_w = fold2_six_word(k);
      }
    }
    // my DMA pieces have landed; after the barrier everyone's have, and everyone has
    // finished reading `buf` (all ds_read results were consumed above)
    if (!(ablate & 8)) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }
  };
  if (half)
    compare_loop(std::true_type{});
  else
    compare_loop(std::false_type{});

  // ---- epilogue: regression (+ boundary) per pair ---------------------------
  if constexpr (MODE == MODE_DIST || ppk_is_mask(MODE) || MODE == MODE_KNN) {
    if (ablate & 1) return;
    if (!FOLD2 && !KS_FUSED && !WIDE_TILE && MODE != MODE_KNN && !wave_active) return;      // (KNN, k-split, wide, FOLD2: every wave takes part in an exchange)
    // the compare stream leaves the wave at priority 0 (it falls through each block, see
    // tools/gen_block_asm.py); the epilogue is the last thing between this workgroup's slot and the next
    // tile, so it runs at the top priority (measured: another -0.5..-1 %)
    __builtin_amdgcn_s_setprio(3);
    // Cut every count register's live range here: whatever the register allocator decides for the
    // epilogue (which has all 128 VGPRs but wants many of them for fp64) must not reach back into
    // the compare loop -- a register spilled "for its whole life" is read-modified-written in
    // scratch at every k, behind an s_waitcnt that also waits for the prefetch DMA.
#pragma unroll
    for (int i = 0; i < W; ++i)
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < TQ; ++q) {
          // a real move: a tied "+v" operand is coalesced back into one live range
          uint32_t t;
          asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"(pw[i][r][q]));
          pw[i][r][q] = t;
        }
    {
      // the loop keeps ONE lane-derived register (voff_ref = 16 * lane); the lane index itself is
      // recovered from it here, opaquely, so that it is not held live across the loop as well
      uint32_t t = voff_ref;
      asm volatile("" : "+v"(t));
      lane_late = (int)(t >> 4);
    }
    // The epilogue reads ~40 dwords of launch parameters the compare loop never touches.  Loaded
    // HERE, through the kernarg segment pointer (DistParams is the 10th argument, after nine
    // pointers; the offset is checked against the code object's metadata by tests/test_abi.py), they
    // do not occupy SGPRs across the
    // loop, where the kernel sits at the register limit.
    const char __attribute__((address_space(4))) *ka =
        (const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    LateParams &p_late = *reinterpret_cast<LateParams *>(ka + V2_PARAMS_KERNARG_OFFSET);
    if constexpr (FOLDH) {
      // ---- the holder pair: the matches the codes cannot see ---------------------------------------------
      // Every value with at most H holders is coded 0 / 1, so a pair that shares such values was counted short by
      // their number at that k.  The database lists what each (pair, k) is owed as 32-bit entries -- hi % 256 |
      // (lo % 32) << 8 | k << 13 | count << 16 -- bucketed like the two-holder pair's events (ppk_db::d_foldh_ent).
      // The dead compare buffers take one 64-bit word per pair of the tile, five 12-bit fields (one per k; a count
      // is at most 64 * sketchsize64 <= 2 048), 64 KB laid out so that lane l of wavefront w reads its sixteen pairs
      // as eight conflict-free 16-byte reads -- [q][r / 2][w * 64 + l][r % 2] -- and the entries are added in with
      // 64-bit LDS atomics.  Barriers, buckets of a strip tile and the wavefronts' exit: as for the two-holder pair.
      static_assert(FOLD2 && PL == 8 && W == 2 && !KSPLIT && !WIDE, "the holder pair is an 8-plane whole-tile kernel");
      static_assert(sizeof(lds) >= 8 * 512 * sizeof(u32x4), "one 64-bit word per pair of the tile");
      const uint32_t tid = (uint32_t)wave * 64u + (uint32_t)lane_late;
      unsigned long long *corr = reinterpret_cast<unsigned long long *>(lds);
      u32x4 zero4;
      zero4.x = zero4.y = zero4.z = zero4.w = 0;
#pragma unroll
      for (int i = 0; i < 2 * TQ; ++i) lds[tid + 512u * i] = zero4;
      __syncthreads();
      {
        const unsigned *off = p_late.fold2_off;
        const uint32_t *ents = reinterpret_cast<const uint32_t *>(p_late.fold2_ev);
        const uint32_t frt = p_late.fold2_rt;
        const uint32_t q_sub = (uint32_t)(q0 >> 5) & 7u;      // strip: which 32 of its ref tile's samples the tile holds
        const int n_buckets = strip ? 8 : 1;
        for (int i = 0; i < n_buckets; ++i) {
          const uint32_t b = strip ? ((uint32_t)(r0 >> 5) + (uint32_t)i) * frt + (uint32_t)(q0 >> 8)
                                   : (uint32_t)(q0 >> 5) * frt + (uint32_t)rt;
          const uint32_t e1 = off[b + 1];
          for (uint32_t e = off[b] + tid; e < e1; e += 512u) {
            const uint32_t ev = ents[e], kk = (ev >> 13) & 7u;
            uint32_t ref_l = ev & 255u, qry_l = (ev >> 8) & 31u;      // hi % 256, lo % 32
            if (strip) {
              if ((ref_l >> 5) != q_sub) continue;
              const uint32_t hi_l = ref_l;
              ref_l = 32u * (uint32_t)i + qry_l;
              qry_l = hi_l & 31u;
            }
            // pair (ref_l, qry_l): wavefront qry_l / 4, q = qry_l % 4, lane (ref_l % 128) / 2, r = ref_l % 2 + 2 * (ref_l / 128)
            const uint32_t slot = ((((qry_l & 3u) * 2u + (ref_l >> 7)) * 512u + (qry_l >> 2) * 64u + ((ref_l & 127u) >> 1)) << 1) + (ref_l & 1u);
            if (kk < 5u)
              __hip_atomic_fetch_add(corr + slot, (unsigned long long)(ev >> 16) << (12u * kk), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        }
      }
      __syncthreads();
      {
        const int cb = p_late.cnt_bits, top = p_late.nk - 1;
#pragma unroll
        for (int q = 0; q < TQ; ++q) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const u32x4 c4 = lds[tid + 512u * (2 * q + h)];
            const uint64_t c[2] = {((uint64_t)c4.y << 32) | c4.x, ((uint64_t)c4.w << 32) | c4.z};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const int r = 2 * h + j;
              if (c[j] != 0) {
                // field k lands where the end-of-k shifts left k's count: bit cnt_bits * (nk - 1 - k)
                uint64_t add = 0;
#pragma unroll
                for (int k = 0; k < 5; ++k)
                  if (k <= top) add += ((c[j] >> (12 * k)) & 4095u) << (cb * (top - k));
                const uint64_t v = (((uint64_t)pw[1][r][q] << 32) | pw[0][r][q]) + add;
                pw[0][r][q] = (uint32_t)v;
                pw[1][r][q] = (uint32_t)(v >> 32);
              }
            }
          }
        }
      }
      __syncthreads();      // (the table copy below lands on the words just read)
      if (!wave_active) return;
    } else if constexpr (FOLD2) {
      // ---- the two-holder pair: the matches the codes cannot see ------------------------------------
      // A value with exactly two holders is coded 0 / 1 like a single-holder one, so the pair (its higher holder as
      // ref, its lower as query) was counted one short at that k.  The database lists these events by (lo / 32,
      // hi / 256) (ppk_db::d_fold2_ev): a tile's bucket is the list of what its pairs are owed.  The compare buffers
      // are dead: their first 32 KB take one dword per pair of the tile, five 6-bit fields (one per k), laid out so
      // that lane l of wavefront w reads its sixteen pairs as four conflict-free 16-byte reads --
      // [q][w * 64 + l][r] -- and the events are added in with LDS atomics.  The barriers are workgroup-wide, so the
      // wavefronts with nothing to compare leave only below.  A strip tile holds the LOWER holders on its lane axis
      // (256 of them: eight buckets) and 32 of the last ref tile's samples on its query axis.
      static_assert(PL == 8 && W == 2 && !KSPLIT && !WIDE, "the two-holder pair is an 8-plane whole-tile kernel");
      const uint32_t tid = (uint32_t)wave * 64u + (uint32_t)lane_late;
      uint32_t *corr = reinterpret_cast<uint32_t *>(lds);
      u32x4 zero4;
      zero4.x = zero4.y = zero4.z = zero4.w = 0;
#pragma unroll
      for (int i = 0; i < TQ; ++i) lds[tid + 512u * i] = zero4;
      __syncthreads();
      {
        const unsigned *off = p_late.fold2_off;
        const uint16_t *evs = p_late.fold2_ev;
        const uint32_t frt = p_late.fold2_rt;
        const uint32_t q_sub = (uint32_t)(q0 >> 5) & 7u;      // strip: which 32 of its ref tile's samples the tile holds
        const int n_buckets = strip ? 8 : 1;
        for (int i = 0; i < n_buckets; ++i) {
          const uint32_t b = strip ? ((uint32_t)(r0 >> 5) + (uint32_t)i) * frt + (uint32_t)(q0 >> 8)
                                   : (uint32_t)(q0 >> 5) * frt + (uint32_t)rt;
          const uint32_t e1 = off[b + 1];
          for (uint32_t e = off[b] + tid; e < e1; e += 512u) {
            const uint32_t ev = evs[e], kk = ev >> 13;
            uint32_t ref_l = ev & 255u, qry_l = (ev >> 8) & 31u;      // hi % 256, lo % 32
            if (strip) {
              if ((ref_l >> 5) != q_sub) continue;
              const uint32_t hi_l = ref_l;
              ref_l = 32u * (uint32_t)i + qry_l;
              qry_l = hi_l & 31u;
            }
            // pair (ref_l, qry_l): wavefront qry_l / 4, q = qry_l % 4, lane (ref_l % 128) / 2, r = ref_l % 2 + 2 * (ref_l / 128)
            const uint32_t slot = (((qry_l & 3u) * 512u + (qry_l >> 2) * 64u + ((ref_l & 127u) >> 1)) << 2) + (ref_l & 1u) + ((ref_l >> 7) << 1);
            if (kk < 5u) __hip_atomic_fetch_add(corr + slot, 1u << (6u * kk), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        }
      }
      __syncthreads();
      {
        const int cb = p_late.cnt_bits, top = p_late.nk - 1;
#pragma unroll
        for (int q = 0; q < TQ; ++q) {
          const u32x4 c4 = lds[tid + 512u * q];
          const uint32_t c[R] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
          for (int r = 0; r < R; ++r) {
            if (c[r] != 0) {
              // field k lands where the end-of-k shifts left k's count: bit cnt_bits * (nk - 1 - k)
              uint64_t add = 0;
#pragma unroll
              for (int k = 0; k < 5; ++k)
                if (k <= top) add += (uint64_t)((c[r] >> (6 * k)) & 63u) << (cb * (top - k));
              const uint64_t v = (((uint64_t)pw[1][r][q] << 32) | pw[0][r][q]) + add;
              pw[0][r][q] = (uint32_t)v;
              pw[1][r][q] = (uint32_t)(v >> 32);
            }
          }
        }
      }
      __syncthreads();      // (the table copy below lands on the words just read)
      if (!wave_active) return;
    }
    uint32_t ks_tile = 0;
    // WIDE: the last group joins the others in the slot; from here on the counts are read from there
    uint32_t wide_slot = 0;
    const uint32_t *wide_src = nullptr;
    if constexpr (WIDE_TILE) {
      wide_slot = __builtin_amdgcn_readfirstlane(*(volatile __attribute__((address_space(3))) uint32_t *)(__attribute__((address_space(3))) void *)(lds + KS_SLOT));
      if (wave_active) {
        wide_park(p_late.wide_groups - 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      wide_src = reinterpret_cast<const uint32_t *>(p_late.wide_slots + (size_t)wide_slot * (size_t)p_late.wide_groups * WIDE_GROUP_U64) +
                 ((uint32_t)wave * 64u + (uint32_t)lane_late);
    }
    if constexpr (KS_FUSED) {
      // ---- k-split job: ONE launch -----------------------------------------------------------------
      // Jobs of less than a round of tiles give every tile to ks_units workgroups (one k, or a half / a
      // quarter of one, each).  A workgroup leaves its 16 partial counts per lane in scratch -- a private
      // 32-byte slot per (tile, unit, thread), so nothing is indexed by row -- and takes a ticket of its
      // tile; the one that draws the last ticket adds the units up, rebuilds the count registers exactly
      // as the whole-tile loop would have left them (k by k: move up one field, add) and runs the same
      // epilogue as every tile of a large job.  Same expressions on the same registers: the distances are
      // bit-identical to the tile kernel's and to the former counts pass + regress_packed_kernel pair,
      // whose second launch (and its gap) this replaces.
      LateParams &pl = p_late;
      const u32x4 pos = lds[KS_SLOT];
      const uint32_t tile = __builtin_amdgcn_readfirstlane(pos.x), unit = __builtin_amdgcn_readfirstlane(pos.y);
      const uint32_t units = pl.ks_units;
      const uint32_t tid = (uint32_t)wave * 64u + (uint32_t)lane_late;
      unsigned *tickets = pl.ks_tickets;
      // partial counts: uint64 [tile][unit][4][512 threads] -- a wavefront's store covers 512 consecutive bytes
      uint64_t *part = reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(pl.ks_tickets) + pl.ks_part_off);
      // Visibility between workgroups, which may run on different XCDs (each with its own L2): every access to
      // the partial counts and to the ticket is an AGENT-scope atomic (relaxed: stores written through, loads
      // served coherently -- the sc1 forms), and the ticket is taken only after this wavefront's stores have
      // completed (s_waitcnt vmcnt(0)) and the workgroup's other wavefronts have said the same at the barrier.
      // That is the compiler's agent-scope release / acquire pair without its two cache-wide operations -- a
      // write-back of the whole L2 (the data here is never left dirty in it) and an invalidate of the whole L2
      // (nothing here is read through a plain load): with a `__threadfence()` per workgroup the 400 workgroups
      // of a 1 000-genome job each flushed and emptied their XCD's L2 and the job took 22 us longer.
      {
        // 16 counts of at most 64 * ks_blocks < 2^16 each
        const uint64_t v0 = (uint64_t)(pw[0][0][0] | (pw[0][1][0] << 16)) | ((uint64_t)(pw[0][2][0] | (pw[0][3][0] << 16)) << 32);
        const uint64_t v1 = (uint64_t)(pw[0][0][1] | (pw[0][1][1] << 16)) | ((uint64_t)(pw[0][2][1] | (pw[0][3][1] << 16)) << 32);
        const uint64_t v2 = (uint64_t)(pw[0][0][2] | (pw[0][1][2] << 16)) | ((uint64_t)(pw[0][2][2] | (pw[0][3][2] << 16)) << 32);
        const uint64_t v3 = (uint64_t)(pw[0][0][3] | (pw[0][1][3] << 16)) | ((uint64_t)(pw[0][2][3] | (pw[0][3][3] << 16)) << 32);
        uint64_t *mine = part + ((size_t)tile * units + unit) * (4 * NW * 64) + tid;
        if (EXP && (ablate & 256)) {
          // (experiments build, bit 256, TIMING ONLY: the hand-over through the XCD's own L2 -- plain stores, an L2
          // ticket, plain reloads -- which is right only if every unit of a tile runs on one XCD, something the
          // dispatch order gives today and nothing promises: what trusting it could win)
          mine[0] = v0;
          mine[NW * 64] = v1;
          mine[2 * NW * 64] = v2;
          mine[3 * NW * 64] = v3;
        } else {
          __hip_atomic_store(mine, v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(mine + NW * 64, v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(mine + 2 * NW * 64, v2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(mine + 3 * NW * 64, v3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wavefront's stores are done
      __syncthreads();
      if (tid == 0) {
        const unsigned t = (EXP && (ablate & 256))
                               ? __hip_atomic_fetch_add(tickets + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
                               : __hip_atomic_fetch_add(tickets + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *reinterpret_cast<volatile unsigned *>(&lds[KS_SLOT]) = t;
      }
      __syncthreads();
      const unsigned ticket = *reinterpret_cast<volatile unsigned *>(&lds[KS_SLOT]);
      __syncthreads();                                       // (read by all before the table copy below may land on it)
      if (ticket + 1 != units) return;                       // another workgroup will fit this tile
      if (tid == 0) __hip_atomic_store(tickets + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // every launch leaves the counters at zero
      ks_tile = tile;
    }
    // the tile's partial counts -> the count registers the whole-tile loop would have left (k by k: move up one
    // field, add the k's pieces).  The counts come from memory, not from this XCD's L2 (agent-scope loads): a
    // round trip each, so a tile of whole k (at most 5) has ALL its loads in flight at once (40 VGPRs, free
    // at this point), others two k at a time; the caller issues this behind the epilogue's table copy, which
    // does not depend on it.
    auto ks_reload = [&]() __attribute__((always_inline)) {
      if constexpr (KS_FUSED) {
        LateParams &pl = p_late;
        const int slices = pl.k_split, nkk = pl.nk, up = 32 - pl.cnt_bits;
        const uint32_t tid = (uint32_t)wave * 64u + (uint32_t)lane_late;
        uint64_t *src = reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(pl.ks_tickets) + pl.ks_part_off) +
                        (size_t)ks_tile * pl.ks_units * (4 * NW * 64) + tid;
#pragma unroll
        for (int i = 0; i < W; ++i)
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < TQ; ++q) pw[i][r][q] = 0;
#define PPK_KS_MOVE_UP()                                                                   \
  _Pragma("unroll") for (int r = 0; r < R; ++r) _Pragma("unroll") for (int q = 0; q < TQ; ++q) { \
    _Pragma("unroll") for (int i = W - 1; i > 0; --i)                                      \
        pw[i][r][q] = __builtin_amdgcn_alignbit(pw[i][r][q], pw[i - 1][r][q], up);         \
    pw[0][r][q] <<= pl.cnt_bits;                                                           \
  }
#define PPK_KS_ADD(cq, q)                                                \
  {                                                                      \
    const uint32_t a_ = (uint32_t)(cq), b_ = (uint32_t)((cq) >> 32);    \
    pw[0][0][q] += a_ & 0xffffu;                                         \
    pw[0][1][q] += a_ >> 16;                                             \
    pw[0][2][q] += b_ & 0xffffu;                                         \
    pw[0][3][q] += b_ >> 16;                                             \
  }
#define PPK_KS_LOAD(unit_, q)                                                                          \
  ((EXP && (ablate & 256)) ? src[(size_t)(unit_) * (4 * NW * 64) + (q) * NW * 64]                       \
                           : __hip_atomic_load(src + (size_t)(unit_) * (4 * NW * 64) + (q) * NW * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        if (nkk <= 5 && slices == 1) {
          uint64_t c[5][TQ];
#pragma unroll
          for (int k = 0; k < 5; ++k)
            if (k < nkk) {      // wave-uniform
#pragma unroll
              for (int q = 0; q < TQ; ++q) c[k][q] = PPK_KS_LOAD(k, q);
            }
#pragma unroll
          for (int k = 0; k < 5; ++k) {
            if (k < nkk) {
              if (k) {
                PPK_KS_MOVE_UP()
              }
#pragma unroll
              for (int q = 0; q < TQ; ++q) PPK_KS_ADD(c[k][q], q)
            }
          }
        } else {
          uint64_t c[2][4][TQ];
#pragma unroll
          for (int h = 0; h < 4; ++h)
            if (h < slices) {
#pragma unroll
              for (int q = 0; q < TQ; ++q) c[0][h][q] = PPK_KS_LOAD(h, q);
            }
#pragma unroll 1
          for (int k2 = 0; k2 < nkk; k2 += 2) {
#pragma unroll
            for (int par = 0; par < 2; ++par) {
              const int k = k2 + par;
              if (k < nkk) {
                if (k + 1 < nkk) {
#pragma unroll
                  for (int h = 0; h < 4; ++h)
                    if (h < slices) {
#pragma unroll
                      for (int q = 0; q < TQ; ++q) c[par ^ 1][h][q] = PPK_KS_LOAD((k + 1) * slices + h, q);
                    }
                }
                if (k) {
                  PPK_KS_MOVE_UP()
                }
#pragma unroll
                for (int h = 0; h < 4; ++h)
                  if (h < slices) {
#pragma unroll
                    for (int q = 0; q < TQ; ++q) PPK_KS_ADD(c[par][h][q], q)
                  }
              }
            }
          }
        }
#undef PPK_KS_MOVE_UP
#undef PPK_KS_ADD
#undef PPK_KS_LOAD
      }
    };
    auto epilogue = [&](LateParams &p) {
    const int ablate_l = EXP ? p.ablate : 0;      // (experiments build only)
    int cr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) cr[r] = (ref_clu && ref_of(r) < p.n_ref) ? ref_clu[ref_of(r)] : 0;
    unsigned n_fail_wave = 0;   // failed fits of this wavefront: ONE atomic at the end
    uint32_t knn_bits[MODE == MODE_KNN ? TQ : 1][R];   // MODE_KNN: distance bits of the 16 pairs, ~0 = no pair
    if constexpr (MODE == MODE_KNN) {
#pragma unroll
      for (int q = 0; q < TQ; ++q)
#pragma unroll
        for (int r = 0; r < R; ++r) knn_bits[q][r] = 0xffffffffu;
    }
    // ---- interior tiles of the default sketch shape -------------------------------------------
    // Almost every tile of a large job lies off the diagonal and inside the band, holds 5 k of 11-bit
    // counts and has one cluster pair (checked below).  Such a tile needs no per-pair validity, cluster
    // or band arithmetic, and its 80 (E, F) look-ups per lane do not go to memory at all.  What the
    // epilogue costs is its DURATION (while a workgroup is in it the CU runs on the other workgroup's
    // wavefronts alone), and with the table in memory that was 16 dependent round trips of divergent
    // 16-byte gathers, 640 instructions of 64 different lines per tile (measured: the same gathers with
    // lane-uniform addresses make the kernel 2.7 % faster; halving the epilogue's VALU work changes
    // nothing; more gathers in flight make it slower).
    // Instead the workgroup copies the table's rows for counts 0..1023 -- 5 x 16 KB = exactly the 80 KB
    // it owns, its compare buffers being dead -- into LDS with 80 one-KB DMA pieces and every look-up is
    // a ds_read_b128.  Count 1024 (every bin equal) wraps to row 0, whose entry is always the NaN
    // sentinel (J = 0 is below the floor), so such a pair takes the general path like any failed fit.
    // Same expressions, same order as fit_packed: same bits.
    bool interior = false;
    size_t cp_tile = 0;      // the tile's one cluster pair: its block of the table (entries)
    if constexpr (LDS_TABLE) {
      interior = p.lut32 && p.nk >= 3 && p.nk <= 5 && p.cnt_bits == 11 && p.lut_kstride == 1025 &&
                 !strip && !half && p.lds_table && r0 + V2_RT <= p.r_limit && q0 >= qb &&
                 q0 + V2_QT <= qe && (!p.self || r0 >= q0 + V2_QT);      // workgroup-uniform
      if constexpr (KS_FUSED) {
        // A k-split job fits ONE tile per workgroup with nothing else on the CU to hide behind, and its tiles
        // are mostly diagonal or band-edge ones: the general statement's sixteen dependent rounds of divergent
        // gathers were 25 - 30 us of such a job's 80.  Here every tile but the strip ones takes the LDS table;
        // pairs that do not exist (r <= q, padding, outside the band, the uncompared half of a half tile) are
        // fitted like the others and simply not written, and only a REAL pair with a k below the floor sends
        // its wavefront to the general statement.
        interior = p.lut32 && p.nk >= 3 && p.nk <= 5 && p.cnt_bits == 11 && p.lut_kstride == 1025 && !strip &&
                   p.lds_table;
      }
      if (interior && (ref_clu || qry_clu)) {
        // Several random-match clusters (a real database has ~3, by base composition): the samples of
        // one tile -- one species, neighbours in the database -- almost always share one, and then the
        // tile needs ONE cluster pair's block of the table.  Every wavefront holds the same 256 refs
        // and reads all 32 queries' cluster ids, so all eight reach the same verdict without talking.
        const int c_ref = ref_clu ? ref_clu[r0] : 0;
        const int c_qry = qry_clu ? qry_clu[q0] : 0;
        bool same = true;
        if (ref_clu) {
#pragma unroll
          for (int r = 0; r < R; ++r) same = same && cr[r] == c_ref;
        }
        if (qry_clu) {
          for (int j = 1; j < V2_QT; ++j) same = same && qry_clu[q0 + j] == c_qry;      // scalar loads
        }
        interior = __all(same);
        cp_tile = (size_t)(c_ref * p.n_clu + c_qry) * p.lut_cpstride;
      }
    }
    const bool table_in_lds = interior;      // (a wavefront may still leave the interior path: `interior` is cleared)
    // MODE_*_ROWS: the queries whose rows the interior path has staged before the wavefront left it (the general
    // statement then fits every query again and rewrites the same mask words, but must not reserve their rows twice)
    [[maybe_unused]] int rows_done = 0;      // wave-uniform
    if constexpr (KS_FUSED && !KS_MEM) {
      if (!interior && wave_active) ks_reload();
    }
    if constexpr (LDS_TABLE) {
    if (interior) {
      {
        const char *tab = reinterpret_cast<const char *>(lut + p.lut_total + 2 * cp_tile) + 16 * lane_late;
        constexpr int PIECES = TAB_U4 / 64 / NW;      // 10 one-KB pieces per wavefront
#pragma unroll
        for (int t = 0; t < PIECES; ++t) {
          const int piece = wave * PIECES + t;        // k = piece / 16, rows 64 * (piece % 16) ..
          if (ablate_l & 64) {
            // (bit 64, measurement only: what the table copy costs -- an upper bound on what issuing part of
            // it under the last compare block could win; the look-ups then read whatever the buffers hold)
          } else if ((piece >> 4) < p.nk) {
            __builtin_amdgcn_global_load_lds(PPK_GPTR(tab + (size_t)(piece >> 4) * (1025 * 16) + (piece & 15) * 1024),
                                             PPK_LPTR(lds + piece * 64), 16, 0, 0);
          } else if ((piece & 15) == 0 && lane_late == 0) {
            // 3 or 4 k: the count registers are shifted up to the 5-k layout below, the missing k read
            // count 0 of their own block, and that row holds (1, 1): a factor that changes no bit
            *reinterpret_cast<f64x2 *>(lds + piece * 64) = f64x2{1.0, 1.0};
          }
        }
        if constexpr (KS_FUSED) {
          if (wave_active) ks_reload();      // its loads travel beside the table copy
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
      if constexpr (KS_FUSED) {
        if (!wave_active) return;      // it has copied its share of the table
      }
      // two register sets of 5 look-ups: pair b+1's are in flight while pair b is finished (three sets
      // measure the same, four spill)
      constexpr int SETS = 2;
      f64x2 ef[SETS][5];
      const char __attribute__((address_space(3))) *ltab =
          (const char __attribute__((address_space(3))) *)(__attribute__((address_space(3))) void *)lds;
      const int up = 11 * (5 - p.nk);      // 0 with the default 5 k
      auto gather = [&](int b, f64x2 (&e)[5]) {
        const uint64_t v = (((uint64_t)pw[1][b & 3][b >> 2] << 32) | pw[0][b & 3][b >> 2]) << up;
        const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
        // k at bit 11 * (4 - k) of the 55-bit register; byte offset = (count mod 1024) * 16
        const uint32_t o0 = (hi >> 8) & 0x3ff0u;
        const uint32_t o1 = (hi << 3) & 0x3ff0u;
        const uint32_t o2 = (__builtin_amdgcn_alignbit(hi, lo, 22) << 4) & 0x3ff0u;
        const uint32_t o3 = (lo >> 7) & 0x3ff0u;
        const uint32_t o4 = (lo << 4) & 0x3ff0u;
        typedef const f64x2 __attribute__((address_space(3))) *LP;
        e[0] = *reinterpret_cast<LP>(ltab + o0);
        e[1] = *reinterpret_cast<LP>(ltab + 16384 + o1);
        e[2] = *reinterpret_cast<LP>(ltab + 32768 + o2);
        e[3] = *reinterpret_cast<LP>(ltab + 49152 + o3);
        e[4] = *reinterpret_cast<LP>(ltab + 65536 + o4);
      };
#pragma unroll
      for (int b = 0; b < SETS - 1; ++b) gather(b, ef[b]);
      float core[R], acc[R];
#pragma unroll
      for (int b = 0; b < R * TQ; ++b) {
        const int q = b >> 2, r = b & 3;
        if (b + SETS - 1 < R * TQ) {
          gather(b + SETS - 1, ef[(b + SETS - 1) % SETS]);
          asm volatile("" ::: "memory");    // the gathers of later pairs stay ahead of everything pair b does
        }
        {
          const f64x2(&e)[5] = ef[b % SETS];
          const double pe = e[0].x * e[1].x * e[2].x * e[3].x * e[4].x;
          const double pf = e[0].y * e[1].y * e[2].y * e[3].y * e[4].y;
          // some lane has a k below the floor: the whole wavefront goes through the general statement below
          bool usable = pe == pe;
          if constexpr (KS_FUSED) {
            const uint32_t rf = (uint32_t)ref_of(r), q32 = (uint32_t)(qw0 + q);
            usable = usable || !(q32 >= (uint32_t)qb && q32 < (uint32_t)qe && rf < (uint32_t)p.r_limit &&
                                 (!p.self || rf > q32) && !(half && r < 2));
          }
          if (!__all(usable) && !(ablate_l & 64)) {
            interior = false;
            if constexpr (ppk_is_rows(MODE)) rows_done = q;
            break;
          }
          fit_finish(pe, pf, core[r], acc[r]);
          // finished HERE (not sunk to the stores, which would keep four pairs' gathers live)
          asm volatile("" : "+v"(core[r]), "+v"(acc[r]));
        }
        if (r != R - 1) continue;
        // the query's four pairs are done: write its rows
        const size_t qq = qw0 + q;   // wave-uniform
        if constexpr (MODE == MODE_DIST) {
          // refs 2l and 2l+1 are adjacent rows: 16 bytes at 8-byte alignment, one global_store_dwordx4
          // (the look-ups wait on lgkmcnt, the stores count in vmcnt: neither waits for the other)
          const size_t rowq = (p.self ? qq * p.n_ref - (qq * (qq + 1)) / 2 - qq - 1 : qq * p.n_ref) - p.row_base;
          float2 *orow = static_cast<float2 *>(out) + (rowq + r0);
          typedef float f32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
          const bool q_in_band = !KS_FUSED || (qq >= qb && qq < qe);      // wave-uniform
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            f32x4_a8 v;
            v.x = core[2 * h];
            v.y = acc[2 * h];
            v.z = core[2 * h + 1];
            v.w = acc[2 * h + 1];
            if constexpr (KS_FUSED) {
              // the pairs that exist: the general statement's own rule
              const uint32_t loc = 2u * (uint32_t)lane_late + 128u * h;
              const uint32_t rf0 = (uint32_t)r0 + loc, q32 = (uint32_t)qq;
              const bool v0 = q_in_band && !(half && h == 0) && rf0 < (uint32_t)p.r_limit && (!p.self || rf0 > q32);
              const bool v1 = q_in_band && !(half && h == 0) && rf0 + 1 < (uint32_t)p.r_limit && (!p.self || rf0 + 1 > q32);
              if (v0 && v1) {
                *reinterpret_cast<f32x4_a8 *>(orow + loc) = v;
              } else {
                if (v0) orow[loc] = make_float2(v.x, v.y);
                if (v1) orow[loc + 1] = make_float2(v.z, v.w);
              }
            } else if (!(ablate_l & 128))      // (measurement only)
              *reinterpret_cast<f32x4_a8 *>(orow + (2u * (uint32_t)lane_late + 128u * h)) = v;
          }
        } else if constexpr (ppk_is_mask(MODE)) {
          uint64_t ball[R];
          // (a k-split tile takes this statement wherever it lies: pairs that do not exist -- r <= q, padding,
          // outside the band, the uncompared half of a half tile -- have no bit, like in the general statement)
          const bool q_in_band_m = !KS_FUSED || (qq >= qb && qq < qe);      // wave-uniform
#pragma unroll
          for (int rr = 0; rr < R; ++rr) {
            bool pred;
            if constexpr (ppk_is_bgmm(MODE)) {
              const ppk_bgmm &bg = *static_cast<const ppk_bgmm *>(out);
              pred = ppk_bgmm_label(core[rr], acc[rr], bg) == bg.within_label;
            } else {
              const float xs = __fdiv_rn(core[rr], p.scale_x), ys = __fdiv_rn(acc[rr], p.scale_y);
              const float sd = ppk_line_dist(xs, ys, p.x_max, p.y_max, p.slope);
              pred = p.inclusive ? (sd <= 0.0f) : (sd < 0.0f);
            }
            if constexpr (KS_FUSED) {
              const uint32_t rf = (uint32_t)ref_of(rr), q32 = (uint32_t)qq;
              pred = pred && !(half && rr < 2) && rf < (uint32_t)p.r_limit && (!p.self || rf > q32);
            }
            ball[rr] = __ballot(pred);
          }
          if (lane_late == 0 && q_in_band_m) {
            uint64_t *mrow = mask_out + (qq - qb) * p.n_rtiles + rt * 4;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const uint64_t e = ball[2 * h], o = ball[2 * h + 1];
              const uint64_t w0 = spread_even((uint32_t)e) | (spread_even((uint32_t)o) << 1);
              const uint64_t w1 = spread_even((uint32_t)(e >> 32)) | (spread_even((uint32_t)(o >> 32)) << 1);
              if (rt * 4 + 2 * h < p.n_rtiles) mrow[2 * h] = w0;
              if (rt * 4 + 2 * h + 1 < p.n_rtiles) mrow[2 * h + 1] = w1;
            }
          }
          if constexpr (ppk_is_rows(MODE)) rows_emit(ball, core, acc, lane_late, (qq - qb) * p.n_rtiles + rt * 4, p.n_rtiles - rt * 4, p);
        } else {
#pragma unroll
          for (int rr = 0; rr < R; ++rr)
            knn_bits[q][rr] = __float_as_uint((p.knn_col ? acc[rr] : core[rr]) + 0.0f);
        }
      }
    }
    }
    if (!interior) {
    if constexpr (KS_FUSED) {
      if (!wave_active) return;
    }
    // A batch = the lane's refs 2h, 2h+1 against query q (2 x nk gathers).  With the default k list
    // the gathers of batch b+1 are issued BEFORE batch b is consumed (two register sets, alternating):
    // the table look-ups are the only memory latency in the epilogue, and there are 8 batches of it.
    constexpr bool PIPE = MODE == MODE_DIST && W == 2 && !WIDE;
    // (the plain distance kernel with the two-dword count register only: the other instantiations have
    // no registers to spare for the second set, and spill)
    const bool pipelined = PIPE && p.lut32 && p.nk == 5;      // wave-uniform
    constexpr int NRB = PIPE ? 1 : 2;      // refs per batch (pipelined: one, 5 gathers = 20 VGPRs per register set)
    constexpr int NB = R * TQ / NRB;       // batches, query-major: b = q * (R / NRB) + r / NRB
    f64x2 ef[2][NRB][5];
    using EpiPack = std::conditional_t<WIDE_TILE, PackWide, std::conditional_t<KS_MEM, PackParts, PackT>>;
    const unsigned long long *parts_src = nullptr;      // KS_MEM: the lane's first partial-count word of this tile
    if constexpr (KS_MEM)
      parts_src = reinterpret_cast<const unsigned long long *>(reinterpret_cast<const char *>(p.ks_tickets) + p.ks_part_off) +
                  (size_t)ks_tile * p.ks_units * KS_UNIT_U64 + ((uint32_t)wave * 64u + (uint32_t)lane_late);
    auto batch_operands = [&](int bq, int br0, size_t (&cpo)[NRB], uint32_t (&loff)[NRB], EpiPack (&pk)[NRB]) {
      const size_t qq = qw0 + bq;
      const int cq = (qry_clu && qq >= qb && qq < qe) ? qry_clu[qq] : 0;
#pragma unroll
      for (int j = 0; j < NRB; ++j) {
        const int r = br0 + j;
        // table index = (cluster of the ref = larger sample, cluster of the query = smaller sample);
        // in a strip launch the lane holds the smaller sample
        const size_t cp = (size_t)(strip ? cq * p.n_clu + cr[r] : cr[r] * p.n_clu + cq) * p.lut_cpstride;
        cpo[j] = cp;
        loff[j] = (uint32_t)cp;
        if constexpr (WIDE_TILE) {
          pk[j].src = wide_src + (size_t)((bq * R + r) * 4) * 512;
        } else if constexpr (KS_MEM) {
          pk[j].src = parts_src + (size_t)bq * 512;
          pk[j].shift = 16 * r;
        } else {
#pragma unroll
          for (int i = 0; i < W; ++i) pk[j].w[i] = pw[i][r][bq];
        }
      }
    };
    if constexpr (PIPE) {
      if (pipelined) {
        size_t cpo[NRB];
        uint32_t loff[NRB];
        PackT pk[NRB];
        batch_operands(0, 0, cpo, loff, pk);
        ef_gather<PackT, NRB, 5>(pk, lut, loff, p, ef[0]);
      }
    }
    uint64_t ball[R];
    bool valid[R], failed[R];
    float core[R], acc[R];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (MODE == MODE_KNN && !wave_active) break;     // nothing was compared: every pair stays "no pair"
      const int q = b / (R / NRB), r0b = (b % (R / NRB)) * NRB;
      const size_t qq = qw0 + q;   // wave-uniform
      const bool in_band = qq >= qb && qq < qe;
      const size_t rowq = (p.self ? qq * p.n_ref - (qq * (qq + 1)) / 2 - qq - 1 : qq * p.n_ref) - p.row_base;
      if constexpr (PIPE) {
        if (pipelined && b + 1 < NB) {
          size_t cpo_n[NRB];
          uint32_t loff_n[NRB];
          PackT pk_n[NRB];
          batch_operands((b + 1) / (R / NRB), ((b + 1) % (R / NRB)) * NRB, cpo_n, loff_n, pk_n);
          ef_gather<PackT, NRB, 5>(pk_n, lut, loff_n, p, ef[(b + 1) & 1]);
          asm volatile("" ::: "memory");    // the gathers of b+1 stay ahead of everything batch b does
        }
      }
      // the fit runs for every lane (counts of padding samples index the table like any other);
      // `valid` only gates what is written
      if (!in_band || (half && r0b < 2)) {   // refs 0/1 of a half tile were not compared: nothing to fit
#pragma unroll
        for (int j = 0; j < NRB; ++j) {
          valid[r0b + j] = failed[r0b + j] = false;
          core[r0b + j] = acc[r0b + j] = 0.0f;
        }
      } else {
        size_t cpo[NRB];
        uint32_t loff[NRB];
        EpiPack pk[NRB];
        float c2[NRB], a2[NRB];
        bool f2[NRB];
        batch_operands(q, r0b, cpo, loff, pk);
#pragma unroll
        for (int j = 0; j < NRB; ++j) {
          const int r = r0b + j;
          const uint32_t rf = (uint32_t)ref_of(r), q32 = (uint32_t)qq;      // sample indices fit 32 bits
          f2[j] = false;
          valid[r] = rf < (uint32_t)p.r_limit && (!p.self || rf > q32);
          if (strip) valid[r] = rf < q32 && rf >= (uint32_t)p.q_begin && rf < (uint32_t)p.q_end;   // band filter on the lane sample
        }
        // the fast path (every k usable in every lane), else pair by pair (unrolled: a rolled loop
        // would index the operand arrays dynamically and push them into scratch)
        bool fast;
        if constexpr (PIPE)
          fast = pipelined ? ef_finish<NRB, 5>(ef[b & 1], c2, a2)
                           : (p.lut32 && fit_rows_fast_anyk<EpiPack, NRB>(pk, lut, loff, p, c2, a2));
        else
          fast = p.lut32 && fit_rows_fast_anyk<EpiPack, NRB>(pk, lut, loff, p, c2, a2);
        if (!fast) {
#pragma unroll
          for (int j = 0; j < NRB; ++j) fit_packed(pk[j], lut, cpo[j], p, c2[j], a2[j], f2[j]);
        }
#pragma unroll
        for (int j = 0; j < NRB; ++j) {
          core[r0b + j] = c2[j];
          acc[r0b + j] = a2[j];
          failed[r0b + j] = f2[j];
        }
      }
      if (r0b + NRB < R || !in_band) continue;     // the query's last batch: write its rows
#pragma unroll
      for (int r = 0; r < R; ++r) n_fail_wave += (unsigned)__popcll(__ballot(valid[r] && failed[r]));
      if constexpr (MODE == MODE_DIST) {
        // refs 2l and 2l+1 are adjacent rows: one 16-byte store when both are written
        float2 *o = static_cast<float2 *>(out);
        if (!strip) {      // workgroup-uniform
          // the query's row block starts at a wave-uniform address; the lane adds a 32-bit offset
          // (row = rowq + ref: per-lane 64-bit index arithmetic was a fifth of the epilogue's VALU work)
          float2 *orow = o + (rowq + r0);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const uint32_t loc = 2u * (uint32_t)lane_late + 128u * h;
            if (valid[2 * h] && valid[2 * h + 1]) {
              // 16 bytes at 8-byte alignment: one global_store_dwordx4 (a 16-byte memcpy is split in two)
              typedef float f32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
              f32x4_a8 v;
              v.x = core[2 * h];
              v.y = acc[2 * h];
              v.z = core[2 * h + 1];
              v.w = acc[2 * h + 1];
              *reinterpret_cast<f32x4_a8 *>(orow + loc) = v;
            } else {
              if (valid[2 * h]) orow[loc] = make_float2(core[2 * h], acc[2 * h]);
              if (valid[2 * h + 1]) orow[loc + 1] = make_float2(core[2 * h + 1], acc[2 * h + 1]);
            }
          }
        } else {
          // strip tile: the lane sample is the smaller index, i.e. the row's "query"
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const size_t rf = ref_of(r);
            if (valid[r])
              o[rf * p.n_ref - (rf * (rf + 1)) / 2 + (qq - rf - 1) - p.row_base] = make_float2(core[r], acc[r]);
          }
        }
      } else if constexpr (ppk_is_mask(MODE)) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          bool pred = false;
          if (valid[r]) {
            if constexpr (ppk_is_bgmm(MODE)) {
              const ppk_bgmm &bg = *static_cast<const ppk_bgmm *>(out);
              pred = ppk_bgmm_label(core[r], acc[r], bg) == bg.within_label;
            } else {
              const float xs = __fdiv_rn(core[r], p.scale_x), ys = __fdiv_rn(acc[r], p.scale_y);
              const float sd = ppk_line_dist(xs, ys, p.x_max, p.y_max, p.slope);
              pred = p.inclusive ? (sd <= 0.0f) : (sd < 0.0f);
            }
          }
          ball[r] = __ballot(pred);
          // strip tile: the lane sample is the row of the mask, the wave-uniform strip sample its
          // column -- one bit in 64 different (zero-initialised) words, set atomically (only the
          // strip tiles touch the words of columns >= r_limit)
          if (strip && pred)
            atomicOr(reinterpret_cast<unsigned long long *>(mask_out) +
                         (ref_of(r) - p.q_begin) * p.n_rtiles + (qq >> 6),
                     1ull << (qq & 63));
        }
      }
      if constexpr (MODE == MODE_KNN) {
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (valid[r]) knn_bits[q][r] = __float_as_uint((p.knn_col ? acc[r] : core[r]) + 0.0f);
      }
      if constexpr (ppk_is_mask(MODE)) {
        // ball[0]/ball[1]: even/odd refs of r0..r0+127; ball[2]/ball[3]: of r0+128..r0+255.
        // Interleave them into the [q][ref/64] bitmask words the compaction pass reads.
        if (lane_late == 0 && !strip) {
          uint64_t *mrow = mask_out + (qq - qb) * p.n_rtiles + rt * 4;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const uint64_t e = ball[2 * h], o = ball[2 * h + 1];
            const uint64_t w0 = spread_even((uint32_t)e) | (spread_even((uint32_t)o) << 1);
            const uint64_t w1 = spread_even((uint32_t)(e >> 32)) | (spread_even((uint32_t)(o >> 32)) << 1);
            if (rt * 4 + 2 * h < p.n_rtiles) mrow[2 * h] = w0;
            if (rt * 4 + 2 * h + 1 < p.n_rtiles) mrow[2 * h + 1] = w1;
          }
        }
        if constexpr (ppk_is_rows(MODE)) {
          // (the rows modes run without strip tiles: plan_grid)
          if (q >= rows_done) rows_emit(ball, core, acc, lane_late, (qq - qb) * p.n_rtiles + rt * 4, p.n_rtiles - rt * 4, p);
        }
      }
    }
    }   // !interior
    if (n_failed && n_fail_wave && lane_late == 0) atomicAdd(n_failed, (unsigned long long)n_fail_wave);
    if constexpr (MODE == MODE_KNN) {
      KnnState *ks = reinterpret_cast<KnnState *>(mask_out);
      uint32_t *thr = reinterpret_cast<uint32_t *>(ks + 1);
      uint32_t *ckeys = static_cast<uint32_t *>(out);
      uint64_t *cvals = reinterpret_cast<uint64_t *>(static_cast<char *>(out) + ks->vals_off);
      const unsigned long long cap = ks->cap;
      uint32_t *ld = reinterpret_cast<uint32_t *>(lds);          // [32 queries][256 refs] distance bits
      uint32_t *lctl = ld + V2_QT * V2_RT;                        // [0] workgroup total, [1..2] its base
      constexpr uint64_t NONE = ~0ull;
      const int knn = p.knn;
      // ref x query job: refs are samples 0 .. n_ref-1, queries n_ref .. n_ref+n_qry-1, in bounds and candidates alike
      const size_t koff = p.self ? 0 : p.n_ref;
      // ---- 1. distances to LDS; the wave's own queries: local top-k by rounds of wave-wide minima ----
      if (table_in_lds) __syncthreads();      // every wavefront is done with the (E, F) table that lives there
      if (wave == 0 && lane_late == 0) lctl[0] = 0;
      uint32_t won[TQ];       // per lane and query: byte r = the round ref r's candidate was extracted in (0xff: none)
      int cq[TQ];             // candidates of query q that pass (wave-uniform): the first cq[q] rounds
      int c1 = 0;
#pragma unroll
      for (int q = 0; q < TQ; ++q) {
        uint32_t *row = ld + (wave * TQ + q) * V2_RT;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          u32x2 v2;
          v2.x = knn_bits[q][2 * h];
          v2.y = knn_bits[q][2 * h + 1];
          *reinterpret_cast<u32x2 *>(row + 2 * lane_late + 128 * h) = v2;
        }
        const size_t qq = qw0 + q;
        won[q] = 0xffffffffu;
        cq[q] = 0;
        if (!wave_active || qq < qb || qq >= qe) continue;      // wave-uniform
        const uint32_t thr_q = __hip_atomic_load(thr + koff + qq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint64_t key[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
          key[r] = knn_bits[q][r] != 0xffffffffu ? (((uint64_t)knn_bits[q][r] << 32) | (uint32_t)ref_of(r)) : NONE;
        uint64_t kth = NONE;
        int round = 0;
        for (; round < knn; ++round) {
          uint64_t m = key[0];
#pragma unroll
          for (int r = 1; r < R; ++r) m = key[r] < m ? key[r] : m;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            const uint64_t v = __shfl_xor(m, o, 64);
            m = v < m ? v : m;
          }
          if (m == NONE) break;                        // fewer than knn pairs here: no bound from this tile
          kth = m;
          const bool pass = (uint32_t)(m >> 32) <= thr_q;    // minima ascend: the passing rounds are a prefix
          // ... and once a minimum is above the bound no later one passes or lowers it: with settled bounds most
          // (query, tile) pairs end here after one round instead of knn
          if (!pass) break;
#pragma unroll
          for (int r = 0; r < R; ++r)
            if (key[r] == m) {                         // keys are unique: one lane, one r
              key[r] = NONE;
              if (pass) won[q] = (won[q] & ~(0xffu << (8 * r))) | ((uint32_t)round << (8 * r));
            }
          cq[q] += pass ? 1 : 0;
        }
        // (only when it improves on what was read: once the bounds have settled no atomic is issued)
        if (round == knn && (uint32_t)(kth >> 32) < thr_q && lane_late == 0) atomicMin(thr + koff + qq, (uint32_t)(kth >> 32));
        c1 += cq[q];
      }
      __syncthreads();
      // ---- 2. the refs: thread t ranks 16 of the 32 queries' distances to ref (t mod 256) ----------
      const int t = wave * 64 + lane_late;
      const int ref_local = t & (V2_RT - 1), qhalf = t >> 8;
      const size_t rf2 = r0 + ref_local;
      uint32_t bits2[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) bits2[j] = ld[(qhalf * 16 + j) * V2_RT + ref_local];
      const uint32_t thr_r = rf2 < p.n_ref ? __hip_atomic_load(thr + rf2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
      uint32_t pass2 = 0;       // bit j: candidate j is among the k smallest of the 16 and passes the bound
      uint32_t kth2 = 0xffffffffu;
      // a distance above the ref's bound neither passes nor changes the rank of one that does, and the knn-th smallest
      // can only lower the bound if it is below it: a wavefront none of whose 64 x 16 distances is within its ref's
      // bound has nothing to rank (the common case once the bounds have settled)
      bool any_within = false;
#pragma unroll
      for (int a = 0; a < 16; ++a) any_within = any_within || bits2[a] <= thr_r;      // (no pair: 0xffffffff <= bound only while the bound is still open, where the ranking has to run anyway)
      if (__ballot(any_within) != 0ull)
#pragma unroll
      for (int a = 0; a < 16; ++a) {
        // rank of a = candidates with a smaller key; within one ref the query index orders ties, and
        // the queries here ascend with j, so (bits, j) is the key
        int rank = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) rank += (bits2[c] < bits2[a] || (bits2[c] == bits2[a] && c < a)) ? 1 : 0;
        const bool is = bits2[a] != 0xffffffffu;
        if (is && rank < knn && bits2[a] <= thr_r) pass2 |= 1u << a;
        if (is && rank == knn - 1) kth2 = bits2[a];
      }
      if (kth2 < thr_r) atomicMin(thr + rf2, kth2);
      const int c2 = __popc(pass2);
      int incl = c2;            // inclusive prefix of c2 over the wave
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane_late >= o) incl += v;
      }
      const int c2_wave = __shfl(incl, 63, 64);
      // ---- 3. one reservation per workgroup -----------------------------------------------------------
      uint32_t off_w = 0;
      if (lane_late == 0) off_w = atomicAdd(lctl, (uint32_t)(c1 + c2_wave));
      off_w = __shfl(off_w, 0, 64);
      __syncthreads();
      if (t == 0) {
        const unsigned long long base = lctl[0] ? atomicAdd(&ks->count, (unsigned long long)lctl[0]) : 0ull;
        lctl[1] = (uint32_t)base;
        lctl[2] = (uint32_t)(base >> 32);
      }
      __syncthreads();
      const unsigned long long base = (((unsigned long long)lctl[2]) << 32) | lctl[1];
      // ---- 4. write: (sample, distance bits << 32 | the other sample) ------------------------------------
      unsigned long long pos = base + off_w;
#pragma unroll
      for (int q = 0; q < TQ; ++q) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const uint32_t rnd = (won[q] >> (8 * r)) & 0xffu;
          if (rnd != 0xffu && pos + rnd < cap) {
            ckeys[pos + rnd] = (uint32_t)(koff + qw0 + q);
            cvals[pos + rnd] = ((uint64_t)knn_bits[q][r] << 32) | (uint32_t)ref_of(r);
          }
        }
        pos += (unsigned long long)cq[q];
      }
      pos = base + off_w + (unsigned long long)c1 + (unsigned long long)(incl - c2);
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (pass2 & (1u << j)) {
          if (pos < cap) {
            ckeys[pos] = (uint32_t)rf2;
            cvals[pos] = ((uint64_t)bits2[j] << 32) | (uint32_t)(koff + q0 + qhalf * 16 + j);
          }
          ++pos;
        }
    }
    };
    if constexpr (WIDE_TILE) {
      // a wavefront with nothing to compare has nothing to fit (the neighbour mode's exchange needs all eight)
      if (wave_active || MODE == MODE_KNN) epilogue(p_late);
      // every wavefront has read its counts back: the slot returns to the pool
      __syncthreads();
      if (threadIdx.x == 0)
        __hip_atomic_fetch_and(p_late.wide_bitmap + (wide_slot >> 5), ~(1u << (wide_slot & 31u)), __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_AGENT);
    } else {
      epilogue(p_late);
    }
  }
