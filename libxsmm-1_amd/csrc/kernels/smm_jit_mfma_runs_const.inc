// smm_jit_mfma_runs_const.inc -- run form on the matrix cores: M, N <= 32, K <= 64, fp32 / fp64, any addressing mode, any leading
// dimensions (the streaming form, XSTREAM: K up to 256 in chunks). The constants; smm_jit_chain.inc and smm_jit_mfma_runs.inc follow.
// The register-tiled run form (smm_jit_shape.inc) spends a product's time on LDS round trips (every k step fetches TM + TN operands per lane
// for TM x TN fma: the LDS pipe is half busy, the waves wait on it) and holds 250-300 registers for a 32^3 fp64 product -- two
// waves per SIMD, spills in the grouped kernel. Here a wave still owns a run (C in the accumulators across its products, the
// products added in batch order), but:
//   * A never touches LDS: v_mfma_{f32,f64}_16x16x4 wants, in lane (l16, lq), the element A(m = 16 mi + l16, k = 4 ks + lq) --
//     sixteen lanes along a column of A, i.e. contiguous in memory for any lda. The fragments of a product are loaded straight
//     from global memory into the registers the instructions read, one k step at a time, and the registers of k step ks are
//     refilled with the NEXT product's right behind the instructions that consumed them;
//   * B (lanes along n would stride through memory) arrives as a flat, coalesced array and is parked in LDS as [n][KSD], KSD
//     chosen so that a fragment fetch is conflict-free;
//   * C goes straight between memory and the accumulators when a run opens and closes (a lane's elements of one register are
//     sixteen consecutive rows of a column).
// Both instructions are k-ordered fma chains with one rounding per product (tools/probe/mfma_f64_chain.hip), K is padded to a
// multiple of four with A = -0 / B = +0 (the product -0 is the identity of the addition for every sum, signs of zeros
// included): C equals the reference's sequential chain bit for bit, as in the register-tiled form.
constexpr int M = XM, N = XN, K = XK;
constexpr int LDA = XLDA, LDB = XLDB, LDC = XLDC;
constexpr int TS = (int)sizeof(T);
constexpr bool F64 = (8 == TS);
typedef T ACC __attribute__((ext_vector_type(4)));
// K goes through the registers and B's image in NCH chunks of KC (a multiple of four): geom::mfma_runs
constexpr geom::MfmaRuns GEO = geom::mfma_runs(TS, N, K, 0 != XSTREAM); // (kernels/smm_jit_geom.h)
constexpr int NCH = GEO.nch, KC = GEO.kc;
constexpr int MI = (M + 15) / 16, NI = (N + 15) / 16, KS = KC / 4, KP4 = KC;
constexpr int KSD = GEO.ksd;                           // row stride of B's image
constexpr int BE = LDB * (N - 1) + K;                  // span of B in memory
constexpr int NLB = (1 == NCH) ? (BE + 63) / 64 : (N * KC + 63) / 64; // one chunk: the flat span; several: N x KC elements per chunk
constexpr int WAVE_LDS = GEO.wave_lds;                 // elements
#define XNROW(r) (F64 ? (lq + 4 * (r)) : (4 * lq + (r)))
