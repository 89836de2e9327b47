// gsalign_amd/csrc/k_tables.hip -- the index tables a context builds once, at gsa_create (and again where MinSeedLength changes): RefSequence
// from the .pac bytes, its 2-bit copy, the Occ blocks, the dense SA, the k-mer jump tables and the presence table.
#include <algorithm>
#include "gsa_ctx.h"
#include "gsa_fm.h"
#include "gsa_seed.h"

// ---------------------------------------------------------------------------
// Dense SA (index upload time).  The on-disk SA keeps every 32nd ROW; a walk from
// sampled row k (SA = p) visits rows with SA p-1, p-2, ... and stops at the next
// sampled row, so the walks started at all sampled rows together touch every row
// exactly once: 2G LF steps in total, one lane per sampled row.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_densify_sa(DevIndex di, u64 n_sa, u32 *d32, u64 *d64)
{
	const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_sa) return;
	u64 k = i << 5;
	u64 p = i == 0 ? di.seq_len : di.sa[i];
	if (d32) d32[k] = (u32)(i == 0 ? 0xFFFFFFFFu : p); else d64[k] = i == 0 ? (u64)-1 : p;
	for (;;) {
		k = fm_lf(di, k); p -= 1;
		if ((k & 31) == 0) break;
		if (d32) d32[k] = (u32)p; else d64[k] = p;
	}
}

// k-mer jump table: entry id = the interval BWT_Search holds after matching the k bases of id
// (base t in bits 2t..2t+1); x2 = 0 when the walk dies earlier (then the stepwise walk is used).
// Needs the dense SA (unique k-mers carry their text position).
__global__ void __launch_bounds__(256) k_build_kmer(DevIndex di, int k, u64 *tab, int e16)
{
	const u64 id = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	if (id >= (1ull << (2 * k))) return;
	FmIntv ik = fm_init(di, (int)(id & 3));                  // base t of the k-mer = bits 2t..2t+1 (same packing as the query in LDS)
	u32 blk = 0; bool alive = true;
	for (int t = 1; t < k && alive; t++) alive = fm_extend(di, ik, (int)((id >> (2 * t)) & 3), blk);
	const u64 loc1 = (alive && ik.x2 == 1) ? fm_locate(di, ik.x0) + 1 : 0;      // unique k-mer: where it is in the text (+1; saves the SA read)
	if (e16) { ((uint4 *)tab)[id] = make_uint4((u32)ik.x0, (u32)ik.x1, alive ? (u32)ik.x2 : 0u, (u32)loc1); return; }
	u64 *e = tab + ((size_t)id << 2);
	e[0] = ik.x0; e[1] = ik.x1; e[2] = alive ? ik.x2 : 0; e[3] = loc1;
}

// RefSequence from the .pac bytes (RestoreReferenceInfo, bwt_index.cpp:229-264; packing: bntseq.c _get_pac -- base f in byte f >> 2, bits ((~f & 3) << 1)): the forward
// strand, then its reverse complement.  A thread takes one pac byte = four bases: one 4-byte store forward, one 4-byte store (when G is a multiple of four; else bytes) backward
__global__ void __launch_bounds__(256) k_unpack_pac(const uint8_t *__restrict__ pac, i64 G, uint8_t *ref)
{
	const i64 G2 = 2 * G;
	for (i64 b = (i64)blockIdx.x * blockDim.x + threadIdx.x; b * 4 < G; b += (i64)gridDim.x * blockDim.x) {
		const u32 v = pac[b];
		const i64 f0 = b * 4;
#pragma unroll
		for (int t = 0; t < 4; t++) {
			const i64 f = f0 + t;
			if (f < G) { const u32 code = (v >> ((~(u32)t & 3u) << 1)) & 3u; ref[f] = (uint8_t)"ACGT"[code]; ref[G2 - 1 - f] = (uint8_t)"TGCA"[code]; }
		}
	}
}
int unpack_pac(gsa_ctx *c, const uint8_t *d_pac, i64 G, uint8_t *d_ref)
{
	const u64 n = ((u64)G + 3) / 4;
	hipLaunchKernelGGL(k_unpack_pac, dim3(grid_for(std::min<u64>(n, 1ull << 28), 256)), dim3(256), 0, c->stream, d_pac, G, d_ref);
	GSA_CHECK(c, hipGetLastError());
	return GSA_OK;
}

// 2-bit packed copy of RefSequence (16 bases per word, LSB first) for the unique-interval text comparison
__global__ void __launch_bounds__(256) k_pack_ref(const uint8_t *__restrict__ ref, u64 n, u32 *out, u64 words)
{
	const u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	if (w >= words) return;
	u32 v = 0;
	for (int t = 0; t < 16; t++) { const u64 p = w * 16 + t; if (p < n) v |= ((u32)gsa_nt4(ref[p]) & 3) << (2 * t); }
	out[w] = v;
}

// (layout of the grouped presence table: comment at pres4_line, gsa_seed.h)
// (grid-stride: a launch holds at most 2^32 - 1 work-items -- the dispatch packet's grid size is 32 bits wide -- and a human index has 6.2 G text
//  positions.  Until round 5 this kernel was launched with one work-item per position: the runtime took the count modulo 2^32, only the first 1.86 G
//  positions of a 3.08 Gbp index were entered, and a 15-mer whose occurrences all lie behind them -- one in five -- was reported ABSENT: the search from
//  such a start ended without a seed.  Found by the first oracle comparison on the native index, tests/human_scale_check.py.)
__global__ void __launch_bounds__(256) k_build_pres(const u32 *__restrict__ ref2, u64 seq_len, int k, u32 *bm)
{
	for (u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; p + (u64)k <= seq_len; p += (u64)gridDim.x * blockDim.x) {
	const u64 w = p >> 4;
	const u64 X = funnel64(ref2[w], ref2[w + 1], ref2[w + 2], (int)(p & 15) << 1) & ((1ull << (2 * k)) - 1);      // the k-mer at p, base t at bits 2t
#pragma unroll
	for (int i = 0; i < 4; i++) {
		// as member i of the group that starts at p - i: its core is X[3-i .. k-i), the rest are X's first 3-i and last i bases
		const u32 line = (u32)((X >> (2 * (3 - i))) & ((1ull << (2 * (k - 3))) - 1));
		const u32 head = (u32)X & ((1u << (2 * (3 - i))) - 1), tail = (u32)(X >> (2 * (k - i))) & ((1u << (2 * i)) - 1);
		const u32 bit = (u32)i * 64u + (head | (tail << (2 * (3 - i))));
		atomicOr(&bm[(size_t)line * 8 + (bit >> 5)], 1u << (bit & 31));
	}
	}
}

// The same table from the k-mer jump table, when that holds k-mers of exactly this length (the default: -slen 15 against a text of more than 4^13
// rows): a k-mer occurs iff its entry's interval is not empty, so 4^k entries are read in order instead of 2G text positions (a human index: 1.07 G
// entries against 6.2 G positions; the scan's four atomics per position were 0.9 s of gsa_create there).
__global__ void __launch_bounds__(256) k_pres_from_kmer(const u64 *__restrict__ tab, int e16, int k, u32 *bm)
{
	const u64 n = 1ull << (2 * k);
	for (u64 X = (u64)blockIdx.x * blockDim.x + threadIdx.x; X < n; X += (u64)gridDim.x * blockDim.x) {
		const bool occurs = e16 ? ((const uint4 *)tab)[X].z != 0u : tab[(X << 2) + 2] != 0ull;
		if (!occurs) continue;
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const u32 line = (u32)((X >> (2 * (3 - i))) & ((1ull << (2 * (k - 3))) - 1));
			const u32 head = (u32)X & ((1u << (2 * (3 - i))) - 1), tail = (u32)(X >> (2 * (k - i))) & ((1u << (2 * i)) - 1);
			const u32 bit = (u32)i * 64u + (head | (tail << (2 * (3 - i))));
			atomicOr(&bm[(size_t)line * 8 + (bit >> 5)], 1u << (bit & 31));
		}
	}
}

// the short companion of the k-mer table (DevIndex::kmer_lo): MinSeedLength bases, when that is less than kmer_k
static int build_kmer_lo(gsa_ctx *c)
{
	const int k = c->prm.MinSeedLength;
	if (c->di.kmer_lo && c->di.kmer_lo_k == k) return GSA_OK;
	c->di.kmer_lo = nullptr; c->di.kmer_lo_k = 0;
	if (!c->di.kmer || k < 8 || k >= c->di.kmer_k || k > 13) return GSA_OK;
	const size_t n = (size_t)1 << (2 * k);
	if (!dev_ensure<u64>(c, c->d_kmer_lo, c->di.kmer_e16 ? n * 2 : n * 4, true)) return GSA_ERR_NOMEM;
	hipLaunchKernelGGL(k_build_kmer, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, c->di, k, c->d_kmer_lo.as<u64>(), c->di.kmer_e16);
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipStreamSynchronize(c->stream));
	c->di.kmer_lo = c->d_kmer_lo.as<u64>(); c->di.kmer_lo_k = k;
	return GSA_OK;
}

int build_presence(gsa_ctx *c)
{
	if (!c->di.ref2) return GSA_OK;                       // (gsa_create sets the parameters after the index is up)
	if (int rcl = build_kmer_lo(c)) return rcl;
	int k = c->prm.MinSeedLength < 16 ? c->prm.MinSeedLength : 16;
	if (k == c->di.pres_k && c->di.pres) return GSA_OK;
	c->di.pres = nullptr; c->di.pres_k = 0;
	if (k < 8) return GSA_OK;                             // short seeds: nearly every k-mer present, nothing to gain
	const size_t words = ((size_t)1 << (2 * (k - 3))) * 8;      // 4^(k-3) lines of 32 bytes
	if (!dev_ensure<u32>(c, c->d_pres, words, true)) return GSA_ERR_NOMEM;
	GSA_CHECK(c, hipMemsetAsync(c->d_pres.p, 0, words * 4, c->stream));
	if (c->di.kmer && c->di.kmer_k == k && c->opt.pres_from_kmer)
		hipLaunchKernelGGL(k_pres_from_kmer, dim3(grid_for(std::min<u64>(1ull << (2 * k), 1ull << 28), 256)), dim3(256), 0, c->stream, c->di.kmer, c->di.kmer_e16, k, c->d_pres.as<u32>());
	else
		hipLaunchKernelGGL(k_build_pres, dim3(grid_for(std::min<u64>(c->di.seq_len, 1ull << 30), 256)), dim3(256), 0, c->stream, c->di.ref2, c->di.seq_len, k, c->d_pres.as<u32>());
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipStreamSynchronize(c->stream));
	c->di.pres = c->d_pres.as<u32>(); c->di.pres_k = k;
	return GSA_OK;
}

// ---- Occ blocks: the reference's interleaved layout (128 rows per 64-byte block: four u64 counts + 128 symbols,
// bwt_search.cpp:69-119) regrouped into 64 rows per 32-byte block (FmBlock, gsa_fm.h) ----
__global__ void __launch_bounds__(256) k_occ_base(const uint4 *__restrict__ src, u64 n_super, int shift, u64 *base)
{
	const u64 sb = (u64)blockIdx.x * 256 + threadIdx.x;
	if (sb >= n_super) return;
	const uint4 *p = src + (((sb << shift) >> 1) << 2);              // (a super-block starts on an even block: a header of the reference)
	const uint4 c0 = p[0], c1 = p[1];
	base[4 * sb] = ((u64)c0.y << 32) | c0.x; base[4 * sb + 1] = ((u64)c0.w << 32) | c0.z; base[4 * sb + 2] = ((u64)c1.y << 32) | c1.x; base[4 * sb + 3] = ((u64)c1.w << 32) | c1.z;
}
__global__ void __launch_bounds__(256) k_occ_relayout(const uint4 *__restrict__ src, u64 n_blocks, const u64 *__restrict__ base, int shift, uint4 *dst)
{
	const u64 b = (u64)blockIdx.x * 256 + threadIdx.x;
	if (b >= n_blocks) return;
	const uint4 *p = src + ((b >> 1) << 2);
	const uint4 c0 = p[0], c1 = p[1], w = p[2 + (b & 1)];
	u64 ca = ((u64)c0.y << 32) | c0.x, cc = ((u64)c0.w << 32) | c0.z, cg = ((u64)c1.y << 32) | c1.x, ct = ((u64)c1.w << 32) | c1.z;
	if (b & 1) {                                                      // the second half of a reference block: its header + its first 64 symbols
		const uint4 w0 = p[2];
		const u64 M = 0x5555555555555555ull;
		u32 n1 = 0, n2 = 0, n3 = 0;
		for (int J = 0; J < 2; J++) {
			const u64 W = J ? (((u64)w0.z << 32) | w0.w) : (((u64)w0.x << 32) | w0.y);
			const u64 lo = W & M, hi = (W >> 1) & M;
			n3 += __popcll(hi & lo); n2 += __popcll(hi & ~lo & M); n1 += __popcll(~hi & lo & M);
		}
		ca += 64 - n1 - n2 - n3; cc += n1; cg += n2; ct += n3;
	}
	if (base) { const u64 *sb = base + ((b >> shift) << 2); ca -= sb[0]; cc -= sb[1]; cg -= sb[2]; ct -= sb[3]; }
	dst[2 * b] = make_uint4((u32)ca, (u32)cc, (u32)cg, (u32)ct);
	dst[2 * b + 1] = w;
}

// `ref_layout` = the index file's bwt words on the device, whole 64-byte blocks, zero-padded
int build_occ(gsa_ctx *c, const void *ref_layout, u64 n_blocks128)
{
	const u64 n_blocks = 2 * n_blocks128;
	const bool wide = c->force_wide || c->di.seq_len >= 0xFFFFFF00ull;
	// super-blocks of 2^31 rows where the counts need them; the forced-wide layout of the test-suite uses 2^16 rows so that small
	// texts have several super-blocks and their relative counts really are relative
	const int shift = c->di.seq_len >= 0xFFFFFF00ull ? 25 : 10;
	if (!dev_ensure<uint4>(c, c->d_bwt, 2 * n_blocks + 4, true)) return GSA_ERR_NOMEM;
	GSA_CHECK(c, hipMemsetAsync(c->d_bwt.p, 0, (2 * n_blocks + 4) * sizeof(uint4), c->stream));
	u64 *base = nullptr;
	if (wide) {
		const u64 n_super = (n_blocks >> shift) + 1;
		if (!dev_ensure<u64>(c, c->d_occ_base, 4 * n_super, true)) return GSA_ERR_NOMEM;
		base = c->d_occ_base.as<u64>();
		hipLaunchKernelGGL(k_occ_base, dim3(grid_for(n_super, 256)), dim3(256), 0, c->stream, (const uint4 *)ref_layout, n_super, shift, base);
		GSA_CHECK(c, hipGetLastError());
	}
	hipLaunchKernelGGL(k_occ_relayout, dim3(grid_for(n_blocks, 256)), dim3(256), 0, c->stream, (const uint4 *)ref_layout, n_blocks, (const u64 *)base, shift, c->d_bwt.as<uint4>());
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipStreamSynchronize(c->stream));
	c->di.bwt = c->d_bwt.as<uint4>(); c->di.occ_base = base; c->di.occ_shift = shift;
	return GSA_OK;
}

// the three steps behind the Occ blocks, in the order gsa_create_opts runs them; gsa_create_from_pac has its dense SA from the sort and calls the other two
int build_ref2(gsa_ctx *c)
{
	const u64 words = c->di.seq_len / 16 + 8;      // (the 64-base text window reads five words from any base)
	if (!dev_ensure<u32>(c, c->d_ref2, words, true)) return GSA_ERR_NOMEM;
	hipLaunchKernelGGL(k_pack_ref, dim3(grid_for(words, 256)), dim3(256), 0, c->stream, c->di.ref, c->di.seq_len, c->d_ref2.as<u32>(), words);
	GSA_CHECK(c, hipGetLastError());
	c->di.ref2 = c->d_ref2.as<u32>();
	return GSA_OK;
}

int densify_sa(gsa_ctx *c, u64 n_sa)
{
	const u64 rows = c->di.seq_len + 1;
	const bool use32 = c->di.seq_len < 0xFFFFFFF0ull && !c->force_wide;
	if (use32) { if (!dev_ensure<u32>(c, c->d_sa_dense, rows + 32, true)) return GSA_ERR_NOMEM; c->di.sa32 = c->d_sa_dense.as<u32>(); c->di.sa64 = nullptr; }
	else { if (!dev_ensure<u64>(c, c->d_sa_dense, rows + 32, true)) return GSA_ERR_NOMEM; c->di.sa64 = c->d_sa_dense.as<u64>(); c->di.sa32 = nullptr; }
	hipLaunchKernelGGL(k_densify_sa, dim3(grid_for(n_sa, 256)), dim3(256), 0, c->stream, c->di, n_sa, (u32 *)c->di.sa32, (u64 *)c->di.sa64);
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipStreamSynchronize(c->stream));
	return GSA_OK;
}

int build_kmer_table(gsa_ctx *c)
{
	// k = ceil(log4(2G)) + 2: nearly all k-mers that occur are unique then (a 10 Mb text: 96 % at k = 14, 86 % at k = 13), so a
	// search is table -> text comparison with no stepwise Occ walk in between -- each Occ step is a round trip AND the
	// heaviest block of the search loop.  Capped at 15 and at a quarter of the free device memory (4^15 x 16 B = 16 GiB
	// of the 288: a human-chromosome-sized text of 5 x 10^8 rows has 34 % unique k-mers at k = 14, 78 % at 15).
	int k = 0; while ((1ull << (2 * k)) < c->di.seq_len) k++;
	k += 2; if (k > 15) k = 15;      // (not beyond the default MinSeedLength: a start whose first 15 bases occur -- presence bitmap -- must find its entry, else it walks base by base)
	{
		size_t fr = 0, tot = 0;
		if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = 8ull << 30; }
		const size_t esz = (c->di.seq_len < 0xFFFFFFF0ull && !c->force_wide) ? 16 : 32;
		while (k > 2 && ((size_t)esz << (2 * k)) > fr / 4) k--;
		if (c->opt.kmer_k) { const int kk = c->opt.kmer_k; if (kk >= 2 && kk <= 15 && ((size_t)esz << (2 * kk)) <= fr / 2) k = kk; }      // (GSA_CREATE_KMER_K; tests: a long table on a short text)
	}
	if (k >= 2) {
		const size_t n = (size_t)1 << (2 * k);
		const int e16 = (c->di.seq_len < 0xFFFFFFF0ull && !c->force_wide) ? 1 : 0;
		{	// (exactly this size: dev_ensure's growth margin would be 16 GiB on the longest table)
			const size_t bytes = (e16 ? n * 2 : n * 4) * sizeof(u64);
			if (c->d_kmer.cap < bytes) {
				if (c->d_kmer.p) { hipFree(c->d_kmer.p); c->d_kmer.p = nullptr; c->d_kmer.cap = 0; }
				size_t got = 0;
				if (void *r = dev_take_reserved(c->device, bytes, &got)) { c->d_kmer.p = r; c->d_kmer.cap = got; }
				else {
				if (hipMalloc(&c->d_kmer.p, bytes) != hipSuccess) { (void)hipGetLastError(); return gsa_fail(c, GSA_ERR_NOMEM, "hipMalloc (k-mer table)"); }
				c->d_kmer.cap = bytes;
				}
			}
		}
		hipLaunchKernelGGL(k_build_kmer, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, c->di, k, c->d_kmer.as<u64>(), e16);
		c->di.kmer_e16 = e16;
		GSA_CHECK(c, hipGetLastError());
		GSA_CHECK(c, hipStreamSynchronize(c->stream));
		c->di.kmer = c->d_kmer.as<u64>(); c->di.kmer_k = k;
	}
	return GSA_OK;
}

int build_dense_sa(gsa_ctx *c, u64 n_sa)
{
	if (int rc = build_ref2(c)) return rc;
	if (int rc = densify_sa(c, n_sa)) return rc;
	return build_kmer_table(c);
}
