// gsalign_amd/csrc/k_dp_stripe.hip -- gap-closing DP (a13), the striped kernel: every job that does not fit the classes
// of k_dp_small.hip (up to 5000 x 5000), and launch_stripes, which batches a list of such jobs by size class.  Cell
// recurrence and traceback automaton: gsa_dp.h; how the jobs are sorted into classes: k_dp.hip.
#include <algorithm>
#include "gsa_ctx.h"
#include "gsa_dp.h"

// ---------------------------------------------------------------------------
// k_dp_stripe: every alignment that does not fit the small kernel.  The n target
// columns are cut into stripes of 64; ONE WAVEFRONT PER PAIR OF STRIPES, the pairs of a
// job on whatever CUs the dispatcher picks (four pairs per workgroup), so a 1.5k x 1.5k
// problem runs on a dozen SIMDs instead of one.
// A wave keeps stripe 2pp in the low 16-bit halves of its registers and stripe 2pp+1, 64
// steps behind, in the high halves: the state (u, v, x, y <= 7 + q + e) fits, and the whole
// recurrence is packed 16-bit VALU (v_pk_add/sub/max/min/mad_u16: one instruction for both
// cells, 29 VALU instructions per step = 14.5 per cell; the one-stripe version had 34).
// On step s lane l handles rows s - l (A) and s - 64 - l (B); the left neighbours arrive by
// one DPP wave rotate of the packed (x | v << 8) pairs, unpacked with per-lane v_perm
// selectors that give lane 0 the boundary row (A) and A's lane 63 (B).  The substitution
// score is a v_perm over two 4-byte tables (one per stripe: my query base against A, C, G,
// T) with a selector per reference row staged in LDS.
// The only dependency between waves is the (x,v) pair of stripe 2pp+1's last column per row:
// it is handed over as self-validating 4-byte granules {tag,x|v<<8}, through LDS inside a
// workgroup and through HBM between workgroups (agent-scope relaxed atomics: write-through /
// L1-bypassing, so no fence and no separate flag; the tag is a 16-bit launch epoch, so the
// granules need no clearing between launches), 8 rows per store; the consumer fetches 8 rows
// per poll, one block ahead.
// Direction NIBBLES go to HBM STRIPE-LOCAL: stripe p owns (m+63) steps of 64 nibbles, eight
// steps per stored dword (assembled by packed multiply-adds), and every traceback tile is
// one contiguous block.
// The wave that finishes last (LDS ticket inside a workgroup, agent-scope release/acquire
// around a global ticket between workgroups) runs the traceback.  It keeps a DP_TILE_ROWS x 64
// tile of the current stripe in LDS and walks it RUN BY RUN: the lanes look ahead along the
// three possible directions (21 cells each) in one LDS read, a ballot gives the length
// of the run the automaton of ksw_backtrack would take step by step, and the run
// is emitted at once.
// Forward progress: a workgroup takes its place in the launch from a TICKET drawn when it starts (not from its
// workgroup index), so the pair pp-1 that pair pp waits for belongs to a workgroup that is already running,
// whatever order the dispatcher starts workgroups in and whatever else competes for the CUs.  The wait is still
// bounded (2 s of wall clock): a launch that trips it is repeated job by job (gsa_align_contig, dp_safe).
// ---------------------------------------------------------------------------
struct StripeJob { i32 job, m, n, P; i64 diroff, bndoff; i32 ctr, first_block; i32 cert, pad_; };      // cert: the job's flag in the band class's list, -1: not in it
#define DP_TILE_ROWS 160        // local diagonals of a traceback tile (64 diagonal steps need 128); a multiple of 8
#define DP_STRIPE_BYTES(M) ((((size_t)(M) + 63 + 7) >> 3) << 8)      // (M + 63) anti-diagonals of 64 nibbles, in blocks of eight
#define DP_C1_PAD 320           // code bytes around the reference fragment: 128 "N" rows in front (stripe B starts 64 steps late, lane 63 another 63), the rest behind
#define DP_TILE_SLACK 16        // the prefetched tile reaches this far past the predicted entry
#ifndef DP_G
#define DP_G 8               // boundary rows per hand-off block (4, 8 or 16)
#endif
// -DGSA_DP_TIMING: in-kernel phase timers for tools/dp_probe.py (single-job launches only)
#ifdef GSA_DP_TIMING
#define DPT(...) __VA_ARGS__
#else
#define DPT(...)
#endif
#define DP_LOOK 21
#define DP_WAIT_TICKS 200000000ull   // bound of a hand-off wait: 2 s of the 100 MHz wall clock
#define DP_CLASS_M 768          // size classes of a long job list: reference fragments above / up to this (see launch_stripes)
#define DP_CLASS_TOP 1536       // ... and, round 5, the upper class cut once more: fragments above this keep the 64 KB layout, (768, 1536] run with 26 KB
#define DP_CLASS_MIN_JOBS 4096
#define DP_PAIR_MIN_JOBS 4096      // a size class of fewer jobs is not paired (option dp_pair = 1): see launch_stripes
#ifndef DP_PRIO_BLOCKS
#define DP_PRIO_BLOCKS 0        // the first so many workgroups of a launch (its largest jobs: the list is sorted by cells) issue at raised priority.  96 until the pairs came:
                                // two A/Bs (profiles/r06_seed_footprint.txt, profiles/dp_pairs_ab.txt) found no difference between 96 and 0, so nothing is raised
#endif
#define DP_LDS_M 3968         // longest reference fragment for which four waves share a workgroup (selectors + 3 boundary columns in 64 KB of LDS)

// packed 16-bit arithmetic on the two halves of a register.  History: round 2 spelled these as inline asm (DP_PK_ASM), because the compiler
// rewrites `min(x, 1)` on packed shorts into per-half compares and selects (five instructions for one).  Since round 4 they come from vector
// builtins (the compiler knows what they are: no `s_nop` behind every one of them, as there was behind each inline-asm statement -- 475 in the
// kernel), and the rewrite is avoided by keeping the constants opaque (DP_OPAQUE: a register the optimiser cannot see through).
typedef unsigned short v2u16 __attribute__((ext_vector_type(2)));
#define V2(X) __builtin_bit_cast(v2u16, (u32)(X))
#define U1(X) __builtin_bit_cast(u32, (v2u16)(X))
__device__ __forceinline__ u32 pk_add(u32 a, u32 b) { return U1(V2(a) + V2(b)); }
__device__ __forceinline__ u32 pk_sub(u32 a, u32 b) { return U1(V2(a) - V2(b)); }
__device__ __forceinline__ u32 pk_max(u32 a, u32 b) { return U1(__builtin_elementwise_max(V2(a), V2(b))); }
__device__ __forceinline__ u32 pk_min(u32 a, u32 b) { return U1(__builtin_elementwise_min(V2(a), V2(b))); }
__device__ __forceinline__ u32 pk_sub_sat(u32 a, u32 b) { return U1(__builtin_elementwise_sub_sat(V2(a), V2(b))); }      // max(a - b, 0)
__device__ __forceinline__ u32 pk_mad(u32 a, u32 b, u32 c) { return U1(V2(a) * V2(b) + V2(c)); }
__device__ __forceinline__ u32 pk_shl(u32 a, u32 sh) { return U1(V2(a) << V2(sh)); }
#define DP_OPAQUE(X) asm volatile("" : "+v"(X))

// SBS = 1, the SIDE-BY-SIDE form: the two halves of a wave hold stripe p of two DIFFERENT jobs X (low) and Y (high), in lockstep.  Each half is an
// ordinary stripe with a 63-step ramp: no lag, no neighbour inside the wave (lane 0 takes both left neighbours from the boundary input), 64 lead-in
// rows, and a wave runs max(m + width - 1) over the halves it has.  The virtual job (X, Y) is sjobs[b], sjobs[b + 1]: tickets, boundary granules and
// the forward pass's LDS are the pair's, direction blocks and results each job's own; the last wave of the pair walks back X, then Y.
// One granule per row carries both jobs' (x, v) of lane 63 under one tag: in the matrix z <= 7 (dp_cell), so v = z - u <= 7 and x = a - (z - 2) <= 2
// (a <= z): a pair fits a byte, two pairs and the epoch tag the 4-byte granule.  Rows past the shorter job's end carry that half's values cut to the
// nibble; like every cell outside a matrix they only ever reach other such cells.
__device__ __forceinline__ u32 dp_pack4(u32 h) { return (h & 0xfu) | ((h >> 4) & 0xf0u) | ((h >> 8) & 0xf00u) | ((h >> 12) & 0xf000u); }          // bytes xX, vX, xY, vY -> nibbles
__device__ __forceinline__ u32 dp_unpack4(u32 g) { return (g & 0xfu) | ((g & 0xf0u) << 4) | ((g & 0xf00u) << 8) | ((g & 0xf000u) << 12); }      // ... and back

template <int WPB, int SBS>
__global__ void __launch_bounds__(64 * WPB) k_dp_stripe(const i32 *__restrict__ blk2job, const StripeJob *__restrict__ sjobs, const uint8_t *__restrict__ pool1, const i64 *__restrict__ off1,
                                                   const uint8_t *__restrict__ pool2, const i64 *__restrict__ off2, uint8_t *dirbase, u32 *bndbase, u32 *ctr,
                                                   uint8_t *revbase, uint8_t *ops, const i64 *__restrict__ ops_off, i32 *ops_len, u32 ep, i32 lds_c1, i32 lds_rows, u32 *err, i32 tick_slot,
                                                   const u32 *__restrict__ cert, u32 cert_tag)
{
	extern __shared__ __attribute__((aligned(16))) u32 C2[];           // the reference fragment as byte selectors of the two stripes' score tables
	// The traceback tile ALIASES the forward pass's LDS (codes + boundary columns): the wave that walks back drew the last
	// ticket of its job, so every stripe of the job -- every other wave of this workgroup -- is through with them.  LDS
	// per workgroup is what limits how many jobs (and which other kernels of the contig) a CU holds.
	uint8_t *tile = (uint8_t *)C2;
	// The LARGEST jobs are the contig's latency floor (the list is sorted by cells: they are the first workgroups): their
	// waves issue ahead of whatever else shares the SIMD.  The mass of smaller jobs behind them does not get that: on a
	// 50 Mb contig they are 10 000 workgroups, and at raised priority they starve the record / small-DP path beside them
	// (its passes ran 5-10x slower), which is the longer path there.
	__shared__ u32 s_bid, s_tick;
	if (threadIdx.x == 0) {
		s_tick = 0;
		const u32 tk = __hip_atomic_fetch_add(&ctr[tick_slot], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (tk == gridDim.x - 1) __hip_atomic_store(&ctr[tick_slot], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // last ticket of this launch: clean for the next one
		s_bid = tk;
	}
	__syncthreads();
	const u32 bid = s_bid;
	if (DP_PRIO_BLOCKS > 0 && bid < (u32)DP_PRIO_BLOCKS) __builtin_amdgcn_s_setprio(3);
	// which job / pair of stripes am I (uniform).  Both tables are read where the host wrote them (pinned memory): two
	// dependent reads across the link cost less than a copy operation in front of the launch
	const StripeJob sj = sjobs[blk2job[bid]];
	const StripeJob sy = SBS ? sjobs[blk2job[bid] + 1] : sj;            // side by side: job Y of the pair (the high halves)
	// The band kernel (k_dp_band.hip) ran in front of this launch: a job it certified has its result, and its workgroups leave here -- behind the launch
	// ticket, which names the job and which every workgroup of a launch must draw (the last one clears it), in front of the job's own ticket, its boundary
	// granules and its direction blocks.  Side by side: only where both partners are certified; else the pair runs as ever and rewrites the same bytes.
	if (sj.cert >= 0 && cert[sj.cert] == cert_tag && (!SBS || (sy.cert >= 0 && cert[sy.cert] == cert_tag))) return;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int m = sj.m, n = sj.n, P = sj.P, PP = SBS ? (P > sy.P ? P : sy.P) : (P + 1) >> 1;      // PP: waves of the (virtual) job
	const int mB = SBS ? sy.m : m, nB = SBS ? sy.n : n;                                    // the high halves' job (lagged: the same one)
	const int mv = SBS ? (m > mB ? m : mB) : m;                         // rows of the virtual job: selectors, boundary columns
	const int pp = ((int)bid - sj.first_block) * WPB + wave;            // stripes 2pp ("A", low halves) and 2pp + 1 ("B", high halves); side by side: stripe pp of X and of Y
	const uint8_t *s1 = pool1 + off1[sj.job], *s2 = pool2 + off2[sj.job];
	const uint8_t *s1B = SBS ? pool1 + off1[sy.job] : s1, *s2B = SBS ? pool2 + off2[sy.job] : s2;
	const size_t pitch = (size_t)DP_STRIPE_BYTES(m);                    // direction nibbles of one stripe: 256 bytes per eight anti-diagonals
	const int nblk = (m + 63 + 7) >> 3;                                 // ... in so many blocks
	const int nblkB = SBS ? (mB + 63 + 7) >> 3 : nblk;
	uint8_t *dir = dirbase + sj.diroff;
	u32 *bnd_in = bndbase + sj.bndoff + (size_t)(pp - 1) * mv, *bnd_out = bndbase + sj.bndoff + (size_t)pp * mv;
	constexpr int LEAD = SBS ? 64 : 128;                                // "N" rows in front of the fragment's selectors
	// C2[LEAD + j] = v_perm selector of step-row j: byte 0 = code of the low halves' reference row j (table: bytes 0-3 of the pair), byte 2 = 4 + code of
	// the high halves' row (table: bytes 4-7) -- lagged: row j - 64 of the same fragment (stripe B lags 64 steps), side by side: row j of Y's fragment --
	// 0x0c ("constant 0") for N, for the rows in front of and behind a fragment (each job's own end), and in bytes 1, 3.  On step s lane l reads entry s - l.
	{
		int fe = (mv + DP_C1_PAD + 63) & ~63; fe = fe < (lds_c1 >> 2) ? fe : (lds_c1 >> 2);
		for (int t = threadIdx.x; t < fe; t += 64 * WPB) {
			const int j = t - LEAD, jb = j - (SBS ? 0 : 64);
			const u32 ca = (j >= 0 && j < m) ? (u32)gsa_nt4(s1[j]) : 4u, cb = (jb >= 0 && jb < (SBS ? mB : m)) ? (u32)gsa_nt4((SBS ? s1B : s1)[jb]) : 4u;
			C2[t] = (ca < 4 ? ca : 0x0cu) | 0x0c000c00u | ((cb < 4 ? 4u + cb : 0x0cu) << 16);
		}
	}
	// WPB > 1: the waves of one workgroup hand their boundary column over through LDS (same granules, tag 0 = not yet)
	u32 *lds_bnd = C2 + (lds_c1 >> 2);
	if (WPB > 1) for (int t = threadIdx.x; t < (WPB - 1) * lds_rows; t += 64 * WPB) lds_bnd[t] = 0;
	u32 *lin = lds_bnd + (size_t)(wave > 0 ? wave - 1 : 0) * lds_rows, *lout = lds_bnd + (size_t)(wave < WPB - 1 ? wave : 0) * lds_rows;
	const bool out_lds = WPB > 1 && wave < WPB - 1;
	// TWO STRIPES PER WAVE, as the two 16-bit halves of every register: u, v, x, y are 0 ... 7 + q + e, so the recurrence runs on
	// packed 16-bit instructions (v_pk_add / max / min / sub: one instruction for both cells).  Stripe B lags 64 steps behind A:
	// on step s lane l holds A's cell (row s - l, column 128 pp + l) and B's cell (row s - 64 - l, column 128 pp + 64 + l), and
	// B's lane 0 takes its left neighbour -- A's lane 63, one step earlier -- from a readlane.
	// Side by side both halves are column 64 pp + l of their own job, row s - l, and either half may be missing (the job has fewer stripes).
	const int tA = SBS ? pp * 64 + lane : pp * 128 + lane, tB = SBS ? tA : tA + 64;
	const bool hasA = SBS ? pp < P : true, hasB = SBS ? pp < sy.P : 2 * pp + 1 < P;
	const int restA = SBS ? n - pp * 64 : n - pp * 128, restB = SBS ? nB - pp * 64 : n - pp * 128 - 64;      // columns from my stripe's first one on
	const int WpB = !hasB ? 0 : (restB < 64 ? restB : 64);
	const int WpA = restA < 64 ? restA : 64;
	const int cqA = tA < n ? gsa_nt4(s2[tA]) : 4, cqB = tB < nB ? gsa_nt4(s2B[tB]) : 4;
	// z = score + q + e (ksw2_alignment.cpp:74-95: match 1, mismatch -1, N 0 -> 7, 5, 6) as a byte table over the reference
	// code, stored XOR 6 so that the selector's "constant 0" is the N row: z = v_perm(tables, selector) ^ 6 in both halves
	u32 tblA = 0, tblB = 0;
#pragma unroll
	for (int cc = 0; cc < 4; cc++) {
		tblA |= (u32)(cqA == 4 ? 0 : (cqA == cc ? 7 ^ 6 : 5 ^ 6)) << (8 * cc);
		tblB |= (u32)(cqB == 4 ? 0 : (cqB == cc ? 7 ^ 6 : 5 ^ 6)) << (8 * cc);
	}
	const u32 uinit2 = SBS ? (tA ? 0x00020002u : 0u) : (tA ? 2u : 0u) | (2u << 16);
	u32 u2 = uinit2, y2 = 0;
	u32 bin = 0, gnext = 0;
	__syncthreads();
	if (pp >= PP) return;                               // (a workgroup's spare waves only helped to stage the fragment)
	const int S_endA = hasA ? m + WpA - 1 : 0, S_endB = hasB ? mB + WpB - 1 : 0;
	const int S_end = SBS ? (S_endA > S_endB ? S_endA : S_endB) : (hasB ? 64 + m + WpB - 1 : m + WpA - 1);      // steps of this wave
	// rows of the boundary column this wave takes in and hands on: side by side, the longest job that has the stripe (the stripe in front of an
	// existing one is full, so the wave in front runs the m + 63 steps those rows need)
	const int mw = SBS ? ((hasA ? m : 0) > (hasB ? mB : 0) ? (hasA ? m : 0) : (hasB ? mB : 0)) : m;
	const int mpub = SBS ? ((pp + 1 < P ? m : 0) > (pp + 1 < sy.P ? mB : 0) ? (pp + 1 < P ? m : 0) : (pp + 1 < sy.P ? mB : 0)) : m;
	// the steady state ends where the first of my stripes runs out of direction blocks
	const int nblk_lo = SBS ? ((hasA ? nblk : 0x7fffffff) < (hasB ? nblkB : 0x7fffffff) ? (hasA ? nblk : 0x7fffffff) : (hasB ? nblkB : 0x7fffffff)) : nblk;
	DPT(const unsigned long long T0c = wall_clock64();)
	u32 *dirA = (u32 *)(dir + (size_t)(SBS ? pp : 2 * pp) * pitch);
	u32 *dirB = SBS ? (u32 *)(dirbase + sy.diroff + (size_t)pp * DP_STRIPE_BYTES(mB)) : (u32 *)(dir + (size_t)(2 * pp + 1) * pitch);
	// boundary granules are fetched ONE BLOCK AHEAD (8 rows per block) so their L2 latency overlaps the block before
	if (pp > 0) {
		const int row = (lane & (DP_G - 1)) < mw ? (lane & (DP_G - 1)) : mw - 1;
		gnext = (WPB > 1 && wave > 0) ? __hip_atomic_load(&lin[row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : __hip_atomic_load(&bnd_in[row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	asm volatile("" :: "v"(gnext));                      // the first prefetch is complete before the loop: inside it, waits then only count stores issued after a prefetch
	const bool pub_stripe = pp < PP - 1;                // (then stripe B is full and its lane 63 owns the boundary column)
	u32 pk2 = 0;                                        // x | v << 8 of my two columns after the current step: bytes xA, vA, xB, vB
	u32 hb = 0;                                         // lanes 0-7: stripe B's boundary column (x | v << 8 of its lane 63), the eight rows of the current block
	const u32 selx = lane ? 0x0c060c04u : (SBS ? 0x0c020c00u : 0x0c040c00u), selv = lane ? 0x0c070c05u : (SBS ? 0x0c030c01u : 0x0c050c01u);      // x, v of (lane - 1 | boundary, A's lane 63) from (rotated pairs, boundary row); side by side lane 0 takes both from the boundary row (bytes xX, vX, xY, vY)
	u32 acc = 0, r0 = 0;                   // direction nibbles of the last four steps (per half, oldest on top); those of the four before
	u32 c1 = 0x00010001u, c2 = 0x00020002u, c4 = 0x00040004u, c7 = 0x00070007u, c16 = 0x00100010u;
	DP_OPAQUE(c1); DP_OPAQUE(c2); DP_OPAQUE(c4); DP_OPAQUE(c7); DP_OPAQUE(c16);
	// one step; K2 is the position inside the 16-step block (a literal in the unrolled body).  GUARD = 1: the first 128 steps (lanes
	// that have not reached row 0 yet are put back to the initial state after every step) and the last blocks (stripe A's
	// direction blocks have an end).  Nothing masks the cells a lane computes outside the matrix -- rows >= m, columns >= n:
	// their values only ever reach other such cells, and their direction nibbles are never read.
// lane K of HB takes the wave-uniform VAL (v_writelane_b32; K a literal / not)
#define DP_WL_LIT(HB, VAL, K) asm("v_writelane_b32 %0, %1, %2" : "+v"(HB) : "s"(VAL), "n"(K));
#define DP_WL_VAR(HB, VAL, K) if (lane == (K)) HB = (VAL);
#define DP_LOADG(MODE, ROW) ((MODE) == 2 ? __hip_atomic_load(&lin[ROW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : __hip_atomic_load(&bnd_in[ROW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
#define DP_STEP(K2, MODE, WSEL, GUARD, WL)                                                                       \
	{                                                                                                           \
		const int s_ = s0 + (K2);                                                                               \
		if (((K2) & (DP_G - 1)) == 0) {                                                                         \
			if ((MODE) == 0) bin = (s_ == 0 && lane == 0) ? 0u : (SBS ? 0x02000200u : 0x200u);    /* t = 0 boundary: x1 = 0, v1 = q, except for the very first cell (:157-164) */ \
			else if (s_ < mw) {                                                                                 \
				/* boundary rows s_ .. s_+DP_G-1 from the pair in front: spin until every granule carries its tag */ \
				const int row = s_ + (lane & (DP_G - 1));                                                       \
				const bool need = lane < DP_G && row < mw;                                                      \
				u32 g = gnext;                                                                                  \
				if (!__all(!need || (g >> 16) == ep)) {      /* (first look outside the loop: its wait only covers the prefetch) */ \
					u32 spins = 0; const unsigned long long t_wait0 = wall_clock64();                          \
					do {                                                                                        \
						if ((++spins & 255) == 0 && (wall_clock64() - t_wait0 > DP_WAIT_TICKS || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) { if (lane == 0) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; } \
						__builtin_amdgcn_s_sleep(1);                                                            \
						if (need) g = DP_LOADG(MODE, row);                                                      \
					} while (!__all(!need || (g >> 16) == ep));                                                  \
				}                                                                                               \
				bin = SBS ? dp_unpack4(g) : g & 0xffffu;                                                                      \
				/* every lane loads (clamped row): an unconditional load lands in gnext without a copy that would wait for it */ \
				const int rown = row + DP_G < mw ? row + DP_G : mw - 1;                                         \
				gnext = DP_LOADG(MODE, rown);                                                                   \
			}                                                                                                   \
		}                                                                                                       \
		/* left neighbours: lane l-1's pair; lane 0 takes (boundary row of A | A's lane 63 for B) */               \
		/* left neighbours: the pairs rotate one lane up (DPP wave_ror:1); lane 0 -- its own byte selectors -- takes the   \
		   boundary row for A and A's lane 63 (row s_ - 64, computed one step ago) for B */                          \
		const u32 bin0 = (u32)__builtin_amdgcn_readlane((int)bin, (K2) & (DP_G - 1));                           \
		const u32 rot = (u32)__builtin_amdgcn_mov_dpp((int)pk2, 0x13C, 0xf, 0xf, true);                         \
		WL(hb, (u32)__builtin_amdgcn_readlane((int)pk2, 63) >> (SBS ? 0 : 16), (K2) & 7)      /* B's lane 63: boundary row s_ - 128 (side by side: both jobs' lane 63, row s_ - 64) */ \
		const u32 x1 = __builtin_amdgcn_perm(rot, bin0, selx), v1 = __builtin_amdgcn_perm(rot, bin0, selv);     \
		const u32 z0 = __builtin_amdgcn_perm(tblB, tblA, (WSEL)) ^ 0x00060006u;                                 \
		const u32 a = pk_add(x1, v1), b = pk_add(y2, u2);                                                       \
		const u32 z1 = pk_max(z0, a), z2 = pk_max(z1, b);                                                       \
		const u32 ta = pk_min(pk_sub(z1, z0), c1), tb = pk_min(pk_sub(z2, z1), c1);      /* a > z; b > max(z, a): the direction is tb ? 2 : ta */ \
		const u32 zc = pk_min(z2, c7);                                                                          \
		const u32 un = pk_sub(zc, v1), vn = pk_sub(zc, u2), zz = pk_sub(zc, c2);                                \
		const u32 xa = pk_sub_sat(a, zz), yb = pk_sub_sat(b, zz);                                               /* x, y */ \
		const u32 fa = pk_min(xa, c1), fb = pk_min(yb, c1);                                                     /* the "x / y is positive" flags (0x08, 0x10 of ksw2) */ \
		/* direction NIBBLES ta | tb << 1 | fa << 2 | fb << 3, four steps per 16-bit half, eight steps per stored dword: the wave \
		   stores 256 bytes per stripe and eight steps (a byte store per step kept the address unit busier than the ALU) */ \
		acc = pk_mad(acc, c16, pk_mad(pk_mad(fb, c2, fa), c4, pk_mad(tb, c2, ta)));                             \
		u2 = un; y2 = yb;                                                                                       \
		pk2 = __builtin_amdgcn_perm(vn, xa, 0x06020400u);      /* bytes xA, vA, xB, vB (values outside the matrix may not fit a byte: cut, not carried into the neighbour) */ \
		if (GUARD) {                                                                                            \
			const u32 keep = (lane <= s_ ? 0xffffu : 0u) | (lane <= s_ - (SBS ? 0 : 64) ? 0xffff0000u : 0u); \
			u2 = (u2 & keep) | (uinit2 & ~keep); y2 &= keep;                                                    \
		}                                                                                                       \
		if (((K2) & 7) == 3) r0 = acc;                                                                  \
		if (((K2) & 7) == 7) {                                                                                  \
			const int blk = s_ >> 3;                                                                            \
			if (hasA && (!(GUARD) || blk < nblk)) dirA[((size_t)blk << 6) + lane] = __builtin_amdgcn_perm(acc, r0, 0x05040100u); \
			if (hasB && (!(GUARD) || (blk >= LEAD / 8 - 8 && blk - (LEAD / 8 - 8) < nblkB))) dirB[((size_t)(blk - (LEAD / 8 - 8)) << 6) + lane] = __builtin_amdgcn_perm(acc, r0, 0x07060302u); \
		}                                                                                                       \
		if (((K2) & 7) == 7 && pub_stripe && s_ >= LEAD + 7) {                                                  \
			/* rows s_-135 .. s_-128 of B's boundary column (side by side: s_-71 .. s_-64 of both) are complete: one store of eight tagged granules */ \
			const int row = s_ - (LEAD + 7) + lane;                                                             \
			if (lane < 8 && row < mpub) {                                                                       \
				if (out_lds) __hip_atomic_store(&lout[row], (ep << 16) | (SBS ? dp_pack4(hb) : hb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); \
				else __hip_atomic_store(&bnd_out[row], (ep << 16) | (SBS ? dp_pack4(hb) : hb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
			}                                                                                                   \
		}                                                                                                       \
	}
	// (three copies of the loop: the first pair has no boundary loads in flight, and keeping it apart keeps its waits off the stores)
#define DP_LOOP(MODE)                                                                                           \
	for (int s0 = 0; s0 < S_end; s0 += 16) {                                                                    \
		const u32 *crow = C2 + LEAD + s0 - lane;               /* my selectors from step s0 on */                  \
		if (s0 + 16 <= S_end) {                                                                                 \
			u32 w[16];                                                                                          \
			_Pragma("unroll") for (int k2 = 0; k2 < 16; k2++) w[k2] = crow[k2];                                   \
			if (s0 >= LEAD && s0 + 16 <= 8 * nblk_lo) {                                                         \
				/* the steady state of a long stripe pair: every lane is under way, every direction block exists */ \
				DP_STEP(0, MODE, w[0], 0, DP_WL_LIT) DP_STEP(1, MODE, w[1], 0, DP_WL_LIT) DP_STEP(2, MODE, w[2], 0, DP_WL_LIT) DP_STEP(3, MODE, w[3], 0, DP_WL_LIT) DP_STEP(4, MODE, w[4], 0, DP_WL_LIT) DP_STEP(5, MODE, w[5], 0, DP_WL_LIT) DP_STEP(6, MODE, w[6], 0, DP_WL_LIT) DP_STEP(7, MODE, w[7], 0, DP_WL_LIT) \
				DP_STEP(8, MODE, w[8], 0, DP_WL_LIT) DP_STEP(9, MODE, w[9], 0, DP_WL_LIT) DP_STEP(10, MODE, w[10], 0, DP_WL_LIT) DP_STEP(11, MODE, w[11], 0, DP_WL_LIT) DP_STEP(12, MODE, w[12], 0, DP_WL_LIT) DP_STEP(13, MODE, w[13], 0, DP_WL_LIT) DP_STEP(14, MODE, w[14], 0, DP_WL_LIT) DP_STEP(15, MODE, w[15], 0, DP_WL_LIT) \
			} else {                                                                                            \
				DP_STEP(0, MODE, w[0], 1, DP_WL_LIT) DP_STEP(1, MODE, w[1], 1, DP_WL_LIT) DP_STEP(2, MODE, w[2], 1, DP_WL_LIT) DP_STEP(3, MODE, w[3], 1, DP_WL_LIT) DP_STEP(4, MODE, w[4], 1, DP_WL_LIT) DP_STEP(5, MODE, w[5], 1, DP_WL_LIT) DP_STEP(6, MODE, w[6], 1, DP_WL_LIT) DP_STEP(7, MODE, w[7], 1, DP_WL_LIT) \
				DP_STEP(8, MODE, w[8], 1, DP_WL_LIT) DP_STEP(9, MODE, w[9], 1, DP_WL_LIT) DP_STEP(10, MODE, w[10], 1, DP_WL_LIT) DP_STEP(11, MODE, w[11], 1, DP_WL_LIT) DP_STEP(12, MODE, w[12], 1, DP_WL_LIT) DP_STEP(13, MODE, w[13], 1, DP_WL_LIT) DP_STEP(14, MODE, w[14], 1, DP_WL_LIT) DP_STEP(15, MODE, w[15], 1, DP_WL_LIT) \
			}                                                                                                   \
		} else {                                                                                                \
			for (int k2 = 0; s0 + k2 < S_end; k2++) DP_STEP(k2, MODE, crow[k2], 1, DP_WL_VAR)                                 \
		}                                                                                                       \
	}
	if (pp == 0) { DP_LOOP(0) } else if (WPB > 1 && wave > 0) { DP_LOOP(2) } else { DP_LOOP(1) }
#undef DP_LOOP
#undef DP_STEP
#undef DP_LOADG
	if (S_end & 7) {
		// the last, partial dwords of the two stripes
		if (S_end & 3) acc = pk_shl(acc, (u32)(4 * (4 - (S_end & 3))) * 0x00010001u);
		if ((S_end & 7) < 4) r0 = acc;
		const int blk = S_end >> 3;
		if (hasA && blk < nblk) dirA[((size_t)blk << 6) + lane] = __builtin_amdgcn_perm(acc, r0, 0x05040100u);
		if (hasB && blk >= LEAD / 8 - 8 && blk - (LEAD / 8 - 8) < nblkB) dirB[((size_t)(blk - (LEAD / 8 - 8)) << 6) + lane] = __builtin_amdgcn_perm(acc, r0, 0x07060302u);
	}
	if (pub_stripe) {
		// the last (partial) block of boundary rows: row m - 1 is lane 63's value after the last step (S_end = m + 127 here; side by side
		// S_end >= mpub + 63, and the rows from mpub on are not handed on)
		if (lane == (S_end & 7)) hb = (u32)__builtin_amdgcn_readlane((int)pk2, 63) >> (SBS ? 0 : 16);
		const int row = (S_end & ~7) - LEAD + lane;
		if (lane <= (S_end & 7) && row >= 0 && row < mpub) {
			if (out_lds) __hip_atomic_store(&lout[row], (ep << 16) | (SBS ? dp_pack4(hb) : hb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			else __hip_atomic_store(&bnd_out[row], (ep << 16) | (SBS ? dp_pack4(hb) : hb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
	DPT(if (pp == 0 && lane == 0) ctr[sj.ctr + 40] = (u32)(wall_clock64() - T0c); if (pp == PP - 1 && lane == 0) ctr[sj.ctr + 41] = (u32)(wall_clock64() - T0c);)
	// ---- ticket: the last wave to finish does the traceback ----
	// A job whose stripes all sit in THIS workgroup (n <= 128 WPB: most of the 22 thousand striped jobs of a human-sized contig)
	// synchronises at workgroup scope with an LDS ticket; agent scope -- stripes in workgroups on other XCDs, whose L2s are not
	// coherent with each other -- means an L2 write-back per stripe and an invalidate in front of the traceback.
	// Longer jobs: the waves of a workgroup first count themselves in LDS, only the last one of each workgroup pays the
	// agent-scope release and draws the job's global ticket (one per workgroup instead of one per wave).
	const bool one_wg = WPB > 1 && PP <= WPB;
	const int first_p = ((int)bid - sj.first_block) * WPB;                 // pairs of this workgroup: first_p .. first_p + mine - 1
	const int mine = PP - first_p < WPB ? PP - first_p : WPB, n_wg = (PP + WPB - 1) / WPB;
	u32 ticket = 0;
	if (WPB > 1) {
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		if (lane == 0) ticket = __hip_atomic_fetch_add(&s_tick, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		ticket = (u32)__builtin_amdgcn_readfirstlane((int)ticket);
		if ((int)ticket != mine - 1) return;
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	}
	if (!one_wg) {
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		if (lane == 0) ticket = __hip_atomic_fetch_add(&ctr[sj.ctr], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		ticket = (u32)__builtin_amdgcn_readfirstlane((int)ticket);
		if ((int)ticket != (WPB > 1 ? n_wg : PP) - 1) return;
		if (lane == 0) ctr[sj.ctr] = 0;                                     // (nobody else looks again: the counters stay clean for the next launch)
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
	}
	DPT(const unsigned long long T1c = wall_clock64(); int ntile = 0, nrun = 0;)
	// side by side: the pair's last wave walks back X, then Y -- the unchanged walker on each job's own direction blocks and result strings
	// (a jump back, not a loop statement: the lagged form then compiles to exactly the code it was)
	int h = 0;
walk_back:
	{
		const int wm = h ? mB : m, wn = h ? nB : n;
		const i32 wjob = h ? sy.job : sj.job;
		const uint8_t *wdir = h ? dirbase + sy.diroff : dir;
		const size_t wpitch = (size_t)DP_STRIPE_BYTES(wm);
		uint8_t *rev = revbase + ops_off[wjob], *op = ops + ops_off[wjob];
		int i = wn - 1, j = wm - 1, state = 0, k = 0;
		// lane l looks at the cell e = l % 21 steps ahead along direction g = l / 21 (0: M, 1: D, 2: I)
		const int g = lane / DP_LOOK, e = lane - g * DP_LOOK;
		const int dlc = g == 2 ? 0 : -e, drl = g == 0 ? -2 * e : -e;
		// The next tile is fetched while the current one is walked: an alignment path runs along the diagonal, so from (i, j)
		// it will enter the stripe to the left near row j - (lc + 1); those diagonals (+-DP_TILE_SLACK for indels on the way)
		// are loaded into registers now and only written to LDS when the walker gets there.  A wrong guess costs nothing but
		// the load: the tile is then fetched the plain way.
		// (a tile = DP_TILE_ROWS / 8 blocks of eight diagonals = 5 KB; block-aligned)
		constexpr int TB_BLKS = DP_TILE_ROWS / 8, TB_VEC = TB_BLKS * 16 / 64;
		static_assert(TB_VEC == 5, "the prefetched tile is five named registers (an array was kept in scratch: 96 bytes per lane)");
		uint4 pf0 = {0, 0, 0, 0}, pf1 = pf0, pf2 = pf0, pf3 = pf0, pf4 = pf0;
#define PF_EACH(X) X(0, pf0) X(1, pf1) X(2, pf2) X(3, pf3) X(4, pf4)
		int pf_sp = -1, pf_lo = 0, pf_hi = -1;
		const int rl_max = wm - 1 + 63;                                      // last local diagonal of a stripe
		const u32 *tile32 = (const u32 *)tile;
		while (i >= 0 && j >= 0) {
			i = __builtin_amdgcn_readfirstlane(i); j = __builtin_amdgcn_readfirstlane(j);
			// tile: stripe sp, local diagonals rl_lo .. rl_hi
			DPT(ntile++;)
			const int sp = i >> 6, rl_hi = j + (i & 63);
			int rl_lo;
			uint4 *dst = (uint4 *)tile;
			if (sp == pf_sp && rl_hi <= pf_hi && rl_hi - pf_lo >= 64) {
				rl_lo = pf_lo;
				DPT(nrun += 1 << 16;)
#define PF_PUT(Q, R) dst[(Q) * 64 + lane] = R;
				PF_EACH(PF_PUT)
#undef PF_PUT
			} else {
				const int b_hi = rl_hi >> 3, b_lo = b_hi - (TB_BLKS - 1) > 0 ? b_hi - (TB_BLKS - 1) : 0;
				rl_lo = b_lo << 3;
				const uint4 *src = (const uint4 *)(wdir + (size_t)sp * wpitch + ((size_t)b_lo << 8));
				const int nvec = (b_hi - b_lo + 1) * 16;
#pragma unroll
				for (int q2 = 0; q2 < TB_VEC; q2++) { const int id = q2 * 64 + lane; if (id < nvec) dst[id] = src[id]; }
			}
			pf_sp = -1;
			{
				const int jp = j - ((i & 63) + 1);
				if (sp > 0 && jp >= 0) {
					int hi = jp + 63 + DP_TILE_SLACK; hi = hi < rl_max ? hi : rl_max;
					const int pb_hi = hi >> 3, pb_lo = pb_hi - (TB_BLKS - 1) > 0 ? pb_hi - (TB_BLKS - 1) : 0;
					const uint4 *src = (const uint4 *)(wdir + (size_t)(sp - 1) * wpitch + ((size_t)pb_lo << 8));
					const int nvec = (pb_hi - pb_lo + 1) * 16;
#define PF_GET(Q, R) { const int id = (Q) * 64 + lane; R = src[id < nvec ? id : 0]; }
					PF_EACH(PF_GET)
#undef PF_GET
					pf_sp = sp - 1; pf_lo = pb_lo << 3; pf_hi = (pb_hi << 3) + 7 < rl_max ? (pb_hi << 3) + 7 : rl_max;
				}
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
			for (;;) {
				// the walker state is wave-uniform: pin it to scalar registers
				i = __builtin_amdgcn_readfirstlane(i); j = __builtin_amdgcn_readfirstlane(j);
				state = __builtin_amdgcn_readfirstlane(state); k = __builtin_amdgcn_readfirstlane(k);
				if (i < 0 || j < 0) break;
				const int lc = i - (sp << 6), rl = j + lc;
				if (lc < 0 || rl < rl_lo) break;                       // left the tile: reload
				const int lc2 = lc + dlc, rl2 = rl + drl;
				const bool valid = lane < 3 * DP_LOOK && lc2 >= 0 && rl2 >= rl_lo && rl2 - lc2 >= 0;
				u32 tmp = 0xffu;
				if (valid) {      // back to ksw2's flag byte (nibble of step k: half k / 4, oldest on top)
					const u32 nb = (tile32[(((rl2 - rl_lo) >> 3) << 6) + lc2] >> ((((rl2 & 7) >> 2) << 4) + ((3 - (rl2 & 3)) << 2))) & 15u;
					tmp = ((nb & 2u) ? 2u : (nb & 1u)) | ((nb & 0xCu) << 1);
				}
				const u32 cur = (u32)__builtin_amdgcn_readfirstlane((int)tmp);
				// the automaton of ksw_backtrack (:38-52) for the current cell ...
				const int S = dp_bt_next(state, cur);
				const int isM = S == 0 ? 1 : 0, isD = (S == 1 || S == 3) ? 1 : 0;
				const int gS = isM ? 0 : (isD ? 1 : 2);
				// ... and for the cells behind it while they keep the same state
				const bool cont = valid && g == gS && (isM ? (tmp & 7) == 0 : (((tmp >> (S + 2)) & 1) != 0 || (int)(tmp & 7) == S));
				const unsigned long long bal = __ballot(cont) >> (gS * DP_LOOK + 1);
				int run = __builtin_ctzll(~bal);
				run = run < DP_LOOK - 1 ? run : DP_LOOK - 1;
				const int L = 1 + run;
				if (lane < L) rev[k + lane] = (uint8_t)(isM ? 'M' : (isD ? 'D' : 'I'));
				k += L; state = S; DPT(nrun++;)
				i -= (isM | isD) ? L : 0; j -= (isM | (1 - isD)) ? L : 0;
			}
		}
		DPT(if (lane == 0) { ctr[sj.ctr + 42] = (u32)(wall_clock64() - T1c); ctr[sj.ctr + 43] = ntile; ctr[sj.ctr + 44] = nrun; ctr[sj.ctr + 45] = (u32)(wall_clock64() - T0c); })
		if (lane == 0) {
			for (; i >= 0; --i) rev[k++] = 'D';
			for (; j >= 0; --j) rev[k++] = 'I';
			ops_len[wjob] = k;
		}
		k = __builtin_amdgcn_readfirstlane(k);
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		for (int q2 = lane; q2 < k; q2 += 64) op[q2] = rev[k - 1 - q2];
	}
	if (SBS && h == 0) { h = 1; goto walk_back; }
}

// Forward wave-steps of a job in the lagged form and of two jobs side by side (S_end of every wave, as the kernel computes it).
static i64 dp_steps_lagged(int m, int n)
{
	const int P = (n + 63) / 64; i64 s = 0;
	for (int pp = 0; 2 * pp < P; pp++) s += 2 * pp + 1 < P ? 64 + m + std::min(n - pp * 128 - 64, 64) - 1 : m + std::min(n - pp * 128, 64) - 1;
	return s;
}
static i64 dp_steps_pair(int mx, int nx, int my, int ny)
{
	const int PX = (nx + 63) / 64, PY = (ny + 63) / 64; i64 s = 0;
	for (int p = 0; p < std::max(PX, PY); p++) s += std::max(p < PX ? mx + std::min(nx - p * 64, 64) - 1 : 0, p < PY ? my + std::min(ny - p * 64, 64) - 1 : 0);
	return s;
}
// One workgroup list of launch_stripes: a job in the lagged form (y < 0) or two jobs side by side; x, y index the job list.
struct DpUnit { i64 cells; size_t x; long long y; };
// The units of one size-class segment [b, e) of `large`.  mode 0: every job alone, in the order of the list.  Otherwise the segment is put in
// (stripe count, m) order, largest first, and neighbours are paired -- mode 1: where the pair costs fewer wave-steps than the two lagged forms
// together; mode 2: always (tests) -- and the head of the unit list is ordered by cells again, as the job list was.
static void dp_make_units(std::vector<LgJob> &large, size_t b, size_t e, int mode, std::vector<DpUnit> &units)
{
	units.clear();
	auto cells = [&](size_t k) { return (i64)large[k].m * large[k].n; };
	if (mode == 0 || e - b < 2) { for (size_t k = b; k < e; k++) units.push_back({ cells(k), k, -1 }); return; }
	std::sort(large.begin() + b, large.begin() + e, [](const LgJob &p, const LgJob &q) {
		const int Pp = (p.n + 63) / 64, Pq = (q.n + 63) / 64;
		return Pp != Pq ? Pp > Pq : (p.m != q.m ? p.m > q.m : p.job < q.job); });
	for (size_t k = b; k < e; ) {
		const bool pair = k + 1 < e && (mode == 2 || dp_steps_pair(large[k].m, large[k].n, large[k + 1].m, large[k + 1].n) < dp_steps_lagged(large[k].m, large[k].n) + dp_steps_lagged(large[k + 1].m, large[k + 1].n));
		if (pair) { units.push_back({ cells(k) + cells(k + 1), k, (long long)(k + 1) }); k += 2; }
		else { units.push_back({ cells(k), k, -1 }); k++; }
	}
	auto by_cells = [&](const DpUnit &p, const DpUnit &q) { return p.cells != q.cells ? p.cells > q.cells : large[p.x].job < large[q.x].job; };
	if (units.size() > 512) std::partial_sort(units.begin(), units.begin() + 256, units.end(), by_cells);
	else std::sort(units.begin(), units.end(), by_cells);
}

// Striped kernel for a list of large jobs on stream `ss` (batches so that the direction bytes of one batch fit the
// budget).  The direction / boundary / ticket buffers are shared: two launches must not be in flight together.
int launch_stripes(gsa_ctx *c, hipStream_t st, std::vector<LgJob> &large, const uint8_t *pool1, const i64 *off1, const uint8_t *pool2, const i64 *off2,
                   uint8_t *ops, const i64 *ops_off, i32 *ops_len, uint8_t *rev, int err_slot)
{
	if (large.empty()) return GSA_OK;
	i32 *mail = c->d_mail.as<i32>();
	// largest first: they are the critical path (only the head of a long list is ordered: the rest fills the machine anyway)
	{
		auto by_cells = [](const LgJob &a, const LgJob &b) { const i64 ca = (i64)a.m * a.n, cb = (i64)b.m * b.n; return ca != cb ? ca > cb : a.job < b.job; };
		if (large.size() > 512) std::partial_sort(large.begin(), large.begin() + 256, large.end(), by_cells);
		else std::sort(large.begin(), large.end(), by_cells);
	}
	// Size classes.  Every workgroup of a launch reserves the LDS the launch's LONGEST reference fragment needs (the code
	// string + three boundary columns): with thousands of jobs that caps the chip at 3 workgroups per CU although almost
	// all of them are small.  Long lists are therefore launched as two kernels, back to back on the stream: fragments
	// above DP_CLASS_M first (the critical ones), the rest behind them with a quarter of the LDS.  Short lists (a bacterial
	// contig: 700 jobs) stay one launch -- there the second kernel would only wait for the longest job of the first.
	// (in front of both: the few fragments above DP_LDS_M, whose boundary columns do not fit LDS -- one wave per workgroup, hand-off
	//  through HBM; they used to drag the whole upper class down to that layout)
	// Round 5: the upper class is cut once more at DP_CLASS_TOP.  Its workgroups hold 16 bytes of LDS per reference row of the class's LONGEST fragment
	// (53 - 64 KB: two or three workgroups per CU), while nine in ten of its jobs are shorter than 1 536 rows (26 KB: six per CU) -- the class ran
	// four rounds of ~0.5 ms on a 250 Mb contig although its longest job needs one.
	size_t n_xl = 0, n_top = large.size(), n_hi = large.size();
	{
		auto it0 = std::stable_partition(large.begin(), large.end(), [](const LgJob &g) { return g.m > DP_LDS_M; });
		n_xl = (size_t)(it0 - large.begin());
		if (large.size() >= DP_CLASS_MIN_JOBS) {
			auto it1 = std::stable_partition(it0, large.end(), [](const LgJob &g) { return g.m > DP_CLASS_TOP; });
			auto it = std::stable_partition(it1, large.end(), [](const LgJob &g) { return g.m > DP_CLASS_M; });
			n_top = (size_t)(it1 - large.begin()); n_hi = (size_t)(it - large.begin());
		}
	}
	for (const LgJob &g : large) if ((((g.m + 63) & ~63) + DP_C1_PAD) * 4 > 150 * 1024) return gsa_fail(c, GSA_ERR_LIMIT, "DP reference-side fragment longer than 38000 bases");
	const i64 budget = 12ll << 30;
	size_t first = 0;
	while (first < large.size()) {
		// descriptors are staged in pinned memory: the upload is asynchronous
		size_t cnt = 0;
		if (c->dp_safe) cnt = 1;      // (retry after a hand-off time-out: one job per launch, every stripe of it resident at once)
		else { size_t l = first; i64 db = 128; while (l < large.size()) { const i64 cells = (((i64)large[l].n + 63) / 64) * (i64)DP_STRIPE_BYTES(large[l].m); if (l > first && db + cells > budget) break; db += cells + 128; l++; } cnt = l - first; }
		// (the early launch and a late one may be in flight together: each has its own table)
		DevBuf &psj = err_slot == M_DPERR3 ? c->p_sj_early : c->p_sj;
		// the segments of this batch: [first, s0) above DP_LDS_M, [s0, st) above DP_CLASS_TOP, [st, s1) above DP_CLASS_M, [s1, first + cnt) below
		const size_t s0 = std::min(std::max(n_xl, first), first + cnt), stp = std::min(std::max(n_top, first), first + cnt), s1 = std::min(std::max(n_hi, first), first + cnt);
		constexpr int NSEG = 4;
		// (a segment is up to two launches: [0] its jobs in the lagged form, [1] its pairs side by side)
		struct Seg { size_t b, e; int mmax, wpb, mpad, lds_rows; size_t dyn_lds; i32 *b2j[2]; i32 nblocks[2]; std::vector<DpUnit> units; } seg[NSEG] = { { first, s0 }, { s0, stp }, { stp, s1 }, { s1, first + cnt } };
		size_t nb_ub = 0;
		for (Seg &sg : seg) {
			sg.mmax = 1;
			for (size_t k = sg.b; k < sg.e; k++) if (large[k].m > sg.mmax) sg.mmax = large[k].m;
			sg.mpad = ((sg.mmax + 63) & ~63) + DP_C1_PAD;      // + the "N" rows in front and behind (see the kernel)
			sg.wpb = sg.mmax <= DP_LDS_M ? 4 : 1;      // reference fragments up to DP_LDS_M bases: four waves (eight stripes) per workgroup, boundary columns through LDS
			sg.lds_rows = (sg.mmax + 15) & ~15;
			sg.dyn_lds = (size_t)sg.mpad * 4 + (sg.wpb > 1 ? (size_t)(sg.wpb - 1) * sg.lds_rows * 4 : 0);      // (one selector dword per row)
			if (sg.dyn_lds < (size_t)DP_TILE_ROWS * 32) sg.dyn_lds = (size_t)DP_TILE_ROWS * 32;      // (the traceback tile -- nibbles -- lives in the same bytes)
			for (size_t k = sg.b; k < sg.e; k++) nb_ub += (size_t)(((large[k].n + 63) / 64 + sg.wpb - 1) / sg.wpb);      // (a wave takes two stripes, or one of each job of a pair)
			// pairs only where four waves share a workgroup: the one-wave class stays as it is (dp_safe: one job per launch, nothing to pair)
			// ... and, by default, only in a class long enough to keep the chip's workgroup slots full (about 1 300 four-wave workgroups): a shorter list is
			// bound by its longest chain of waves, not by instructions, and a pair halves its workgroups and walks back two jobs on one wave -- with every
			// class paired yeast's lists of a few hundred jobs ran 12 % slower per step (3.12 -> 3.50 ms; profiles/dp_pairs_ab.txt section 4).
			// Such a class takes the parent's path untouched: its order, one launch, no second stream.  dp_pair 3 (tests): the rule without this condition
			int mode = sg.wpb == 4 ? c->opt.dp_pair : 0;
			if (mode == 1 && sg.e - sg.b < DP_PAIR_MIN_JOBS) mode = 0;
			dp_make_units(large, sg.b, sg.e, mode == 3 ? 1 : mode, sg.units);
			for (const DpUnit &u : sg.units) { c->dp_stats[0] += u.y >= 0 ? 2 : 1; c->dp_stats[1] += u.y >= 0 ? 2 : 0; }
		}
		// The band class: the near-diagonal jobs of the batch go through k_dp_band first (launch_band); they keep their place in the lists below, and their
		// workgroups leave the striped kernel where the band result is certified.  band_ord: a job's place in the band list (its flag), by place in `large`
		std::vector<i32> band_idx, band_ord(cnt, -1);
		if (c->opt.dp_band && !c->dp_safe) {
			for (size_t k = first; k < first + cnt; k++) {
				const LgJob &g = large[k];
				if (dp_band_eligible(c, g.m, g.n, std::min(dp_steps_lagged(g.m, g.n), dp_steps_pair(g.m, g.n, g.m, g.n) / 2))) band_idx.push_back((i32)k);
			}
			std::sort(band_idx.begin(), band_idx.end(), [&](i32 p, i32 q) { const int sp = large[(size_t)p].m + large[(size_t)p].n, sq = large[(size_t)q].m + large[(size_t)q].n; return sp != sq ? sp > sq : large[(size_t)p].job < large[(size_t)q].job; });
			for (size_t k = 0; k < band_idx.size(); k++) band_ord[(size_t)band_idx[k] - first] = (i32)k;
		}
		const size_t sj_bytes = ((cnt + 1) * sizeof(StripeJob) + (nb_ub + 2) * 4 + 15) & ~(size_t)15;
		if (!pin_ensure<char>(c, psj, sj_bytes + dp_band_table_bytes(band_idx.size()))) return GSA_ERR_NOMEM;
		StripeJob *sj = psj.as<StripeJob>();
		i32 *b2j_all = (i32 *)(sj + cnt + 1);
		BandJob *band_tab = (BandJob *)(psj.as<char>() + sj_bytes);
		i64 dbytes = 128, bwords = 0; i32 nctr = 2 * NSEG; size_t b2j_used = 0, nsj = 0;      // (ctr[0 .. 2 NSEG - 1]: launch tickets of the size classes' two forms)
		for (Seg &sg : seg) {
			for (int form = 0; form < 2; form++) {
				sg.b2j[form] = b2j_all + b2j_used; sg.nblocks[form] = 0;
				for (const DpUnit &u : sg.units) {
					if ((u.y >= 0) != (form == 1)) continue;
					// the table entry of the job / of X and, behind it, of Y
					const int nj = form ? 2 : 1;
					StripeJob s[2];
					for (int q = 0; q < nj; q++) {
						const LgJob &g = large[q ? (size_t)u.y : u.x];
						s[q].cert = band_ord[(q ? (size_t)u.y : u.x) - first]; s[q].pad_ = 0;
						const i64 cells = (((i64)g.n + 63) / 64) * (i64)DP_STRIPE_BYTES(g.m);   // stripe-local direction nibbles
						s[q].job = g.job; s[q].m = g.m; s[q].n = g.n; s[q].P = (g.n + 63) / 64;
						s[q].diroff = dbytes; dbytes += cells + 128;
						s[q].bndoff = 0; s[q].ctr = 0; s[q].first_block = sg.nblocks[form];
					}
					// boundary columns and the ticket are the (virtual) job's
					const int waves = form ? std::max(s[0].P, s[1].P) : (s[0].P + 1) / 2, rows = form ? std::max(s[0].m, s[1].m) : s[0].m;
					s[0].bndoff = bwords; bwords += (i64)((form ? waves : s[0].P) - 1) * rows;
					s[0].ctr = nctr++;
					for (int b = 0; b < (waves + sg.wpb - 1) / sg.wpb; b++) sg.b2j[form][sg.nblocks[form]++] = (i32)nsj;
					for (int q = 0; q < nj; q++) sj[nsj++] = s[q];
				}
				b2j_used += (size_t)sg.nblocks[form];
			}
		}
		const size_t last = first + cnt;
		uint8_t *dir = dev_ensure<uint8_t>(c, c->d_scan2, (size_t)dbytes + 512);
		const size_t bnd_cap0 = c->d_dp_bnd.cap;
		u32 *bnd = dev_ensure<u32>(c, c->d_dp_bnd, (size_t)bwords + 64);
		const size_t ctr_cap0 = c->d_dp_ctr.cap;
		u32 *ctr = dev_ensure<u32>(c, c->d_dp_ctr, (size_t)nctr + 64);
		if (!dir || !bnd || !ctr) return GSA_ERR_NOMEM;
		// boundary granules carry the launch epoch as their tag: cleared only when the buffer is new or the epoch wraps
		c->dp_epoch = (c->dp_epoch + 1) & 0xffffu;
		if (c->dp_epoch == 0 || c->d_dp_bnd.cap != bnd_cap0) { GSA_CHECK(c, hipMemsetAsync(bnd, 0, c->d_dp_bnd.cap, st)); if (c->dp_epoch == 0) c->dp_epoch = 1; }
		// (the ticket counters are put back to zero by the wave that draws the last ticket; the error word lives in the mailbox)
		if (c->d_dp_ctr.cap != ctr_cap0 || c->dp_dirty) { GSA_CHECK(c, hipMemsetAsync(ctr, 0, c->d_dp_ctr.cap, st)); GSA_CHECK(c, hipMemsetAsync(mail + err_slot, 0, 4, st)); c->dp_dirty = false; }
		// (the two classes back to back on one stream.  Side by side on two streams -- the few long jobs at raised priority --
		//  was measured at 250 Mb: same step time, the refinement passes beside them starve instead: the chip is busy either way)
		// (option dp_side: the lower class on a stream of its own -- it then starts with the upper one instead of behind it; the classes share
		//  nothing but the error word: tickets per class, direction / boundary bytes per job)
		const u32 *cert = nullptr; u32 cert_tag = 0;
		if (!band_idx.empty()) { int rc = launch_band(c, st, large, band_idx, band_tab, pool1, off1, pool2, off2, ops, ops_off, ops_len, rev, &cert, &cert_tag); if (rc) return rc; }
		auto blocks_of = [&](int si) { return seg[si].nblocks[0] + seg[si].nblocks[1]; };
		const bool side = c->opt.dp_side && c->stream_aux[3] && blocks_of(NSEG - 1) > 0 && (blocks_of(0) > 0 || blocks_of(1) > 0 || blocks_of(2) > 0);
		// A class's unpaired jobs -- what found no partner in (stripe count, m) order: the odd sizes, the largest among them -- run BESIDE its pairs, on
		// stream_aux[3]: behind each other on one stream, a 250 Mb contig alone waited 2 ms for a few dozen long lagged jobs before its pairs started
		// (one context, every class paired: 11.47 -> 13.32 ms per contig behind each other, 12.68 ms beside; profiles/dp_pairs_ab.txt section 4).  The two launches share nothing but the error word.
		bool beside = false;
		for (const Seg &sg : seg) if (sg.nblocks[0] > 0 && sg.nblocks[1] > 0 && c->stream_aux[3]) beside = true;
		if (side || beside) { GSA_CHECK(c, hipEventRecord(c->ev[24], st)); GSA_CHECK(c, hipStreamWaitEvent(c->stream_aux[3], c->ev[24], 0)); }
		hipStream_t st_main = st;
		for (int si = 0; si < NSEG; si++) {
			const Seg &sg = seg[si];
			hipStream_t st_seg = (side && si == NSEG - 1) ? c->stream_aux[3] : st_main;
			hipStream_t st = (beside && sg.nblocks[1] > 0) ? c->stream_aux[3] : st_seg;      // (of the lagged launch)
			c->dp_stats[2] += sg.nblocks[0] > 0; c->dp_stats[3] += sg.nblocks[1] > 0;
			if (sg.nblocks[0] > 0) {
				if (sg.wpb == 4) hipLaunchKernelGGL((k_dp_stripe<4, 0>), dim3((unsigned)sg.nblocks[0]), dim3(256), sg.dyn_lds, st, (const i32 *)sg.b2j[0], (const StripeJob *)sj, pool1, off1, pool2, off2, dir + 256, bnd, ctr, rev, ops, ops_off, ops_len, c->dp_epoch, (i32)(sg.mpad * 4), (i32)sg.lds_rows, (u32 *)(mail + err_slot), 2 * si, cert, cert_tag);
				else hipLaunchKernelGGL((k_dp_stripe<1, 0>), dim3((unsigned)sg.nblocks[0]), dim3(64), sg.dyn_lds, st, (const i32 *)sg.b2j[0], (const StripeJob *)sj, pool1, off1, pool2, off2, dir + 256, bnd, ctr, rev, ops, ops_off, ops_len, c->dp_epoch, (i32)(sg.mpad * 4), (i32)sg.lds_rows, (u32 *)(mail + err_slot), 2 * si, cert, cert_tag);
			}
			if (sg.nblocks[1] > 0) hipLaunchKernelGGL((k_dp_stripe<4, 1>), dim3((unsigned)sg.nblocks[1]), dim3(256), sg.dyn_lds, st_seg, (const i32 *)sg.b2j[1], (const StripeJob *)sj, pool1, off1, pool2, off2, dir + 256, bnd, ctr, rev, ops, ops_off, ops_len, c->dp_epoch, (i32)(sg.mpad * 4), (i32)sg.lds_rows, (u32 *)(mail + err_slot), 2 * si + 1, cert, cert_tag);
		}
		if (side || beside) { GSA_CHECK(c, hipEventRecord(c->ev[25], c->stream_aux[3])); GSA_CHECK(c, hipStreamWaitEvent(st, c->ev[25], 0)); }
		GSA_CHECK(c, hipGetLastError());
		DPT(GSA_CHECK(c, hipStreamSynchronize(st)); if (cnt == 1) { u32 hh[6]; hipMemcpy(hh, ctr + sj[0].ctr + 40, 24, hipMemcpyDeviceToHost); fprintf(stderr, "[dp] %d x %d: fwd0 %.1f us  fwdlast %.1f us  traceback %.1f us (tiles %u runs %u)  total %.1f us\n", sj[0].m, sj[0].n, hh[0] * 0.01, hh[1] * 0.01, hh[2] * 0.01, hh[3], hh[4], hh[5] * 0.01); })
		if (last < large.size()) {
			// the staging buffer and the direction bytes are reused by the next batch
			i32 *h = c->h_mail;
			GSA_CHECK(c, hipMemcpyAsync(h, mail, MAIL_N * sizeof(i32), hipMemcpyDeviceToHost, st));
			GSA_CHECK(c, hipStreamSynchronize(st));
			if (h[err_slot]) { c->dp_dirty = c->dp_timeout = true; return gsa_fail(c, GSA_ERR_STATE, "internal: DP stripe hand-off timed out"); }
		}
		first = last;
	}
	return GSA_OK;
}
