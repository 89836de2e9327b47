// gsalign_amd/csrc/gsa_index.h -- what the two sorters of the device index builder share (k_index.hip: up to 2^31 - 2 suffixes, one list, 32-bit suffix numbers;
// k_index_wide.hip: more, in batches, 64-bit suffix numbers): the packed text and its readers, the first-pass key, the description of a sort that k_index.hip's
// one derivation half (BWT, Occ counts, samples, the tables of a context) reads.
#ifndef GSA_INDEX_H
#define GSA_INDEX_H
#include "gsa_scan.h"

#define IX_H0 29
#define IX_T 256

static inline unsigned ix_grid(i64 n) { const i64 g = (n + IX_T - 1) / IX_T; return (unsigned)(g < 1 ? 1 : (g > 16384 ? 16384 : g)); }      // (grid-stride kernels: at most 2^22 work-items per launch)

__device__ __forceinline__ u32 ix_pacsym(const uint8_t *__restrict__ pac, i64 q) { return (u32)(pac[q >> 2] >> ((~q & 3) << 1)) & 3u; }
// the 32 bases from p on, first base in the top bits; the words behind the text are zero
__device__ __forceinline__ u64 ix_get32(const u64 *__restrict__ tw, i64 p)
{
	const i64 wi = p >> 5; const int sh = (int)(p & 31) * 2;
	const u64 a = tw[wi], b = tw[wi + 1];
	return sh ? (a << sh) | (b >> (64 - sh)) : a;
}
__device__ __forceinline__ u32 ix_sym(const u64 *__restrict__ tw, i64 p) { return (u32)(tw[p >> 5] >> (62 - 2 * (int)(p & 31))) & 3u; }
// the 63-bit first-pass key of suffix i: {its first IX_H0 bases, padded with A | min(bases left, IX_H0)} (k_index.hip, END OF TEXT)
__device__ __forceinline__ u64 ix_key0(const u64 *__restrict__ tw, i64 i, i64 S) { const i64 l = S - i; return ((ix_get32(tw, i) >> 6) << 5) | (u64)(l < IX_H0 ? l : IX_H0); }

// T, 2 bits per base, 32 bases per word: the forward strand from .pac, behind it its reverse complement (the text gsah_build_index forms), zeros behind that
static __global__ void __launch_bounds__(IX_T) k_ix_pack(const uint8_t *__restrict__ pac, i64 G, i64 S, u64 *__restrict__ tw, i64 n_tw)
{
	for (i64 w = (i64)blockIdx.x * IX_T + threadIdx.x; w < n_tw; w += (i64)gridDim.x * IX_T) {
		u64 v = 0; const i64 p0 = w * 32;
#pragma unroll 8
		for (int k = 0; k < 32; k++) {
			const i64 p = p0 + k;
			u32 s = 0;
			if (p < G) s = ix_pacsym(pac, p); else if (p < S) s = 3u - ix_pacsym(pac, S - 1 - p);
			v |= (u64)s << (62 - 2 * k);
		}
		tw[w] = v;
	}
}

// the builder's device arrays: all freed when the call returns, whichever way (gsa_create_from_pac takes SA out first: release)
struct IxBufs {
	hipStream_t st; std::vector<void *> p;
	~IxBufs() { free_all(); }
	void free_all() { if (p.empty()) return; (void)hipStreamSynchronize(st); for (void *q : p) (void)hipFree(q); p.clear(); (void)hipGetLastError(); }
	void release(void *q) { for (size_t k = 0; k < p.size(); k++) if (p[k] == q) { p.erase(p.begin() + (long)k); return; } }
	template <class T> bool get(T **out, size_t n) { void *q = nullptr; if (hipMalloc(&q, (n ? n : 1) * sizeof(T) + 256) != hipSuccess) { (void)hipGetLastError(); return false; } p.push_back(q); *out = (T *)q; return true; }
};

// A sort, begun (ix_begin) and finished (ix_sort_narrow / ix_sort_wide): SA (n + 32 entries of 4 or 8 bytes: the size of a context's dense SA, build_dense_sa), the packed
// text, the .pac bytes, the status words {length of the narrow sorter's next list, primary}, the Occ carries (two sets of four: ix_bwt_occ); d_bwt is zeroed for the
// BWT / Occ passes (whole 64-byte blocks of the file layout and one more: what build_occ reads), d_sa is there when asked for
struct IxBuilt {
	IxBufs B;
	i64 G = 0, S = 0, n = 0, n_tw = 0, n_words = 0, n_blk = 0, n_bwt = 0, n_sa = 0, k_end = 0; i32 rounds = 0; i64 batches = 0, active = 0;      // active: the suffixes that still tie after the first pass (the wide sorter's longest list)
	uint8_t *d_pac = nullptr; u64 *tw = nullptr, *d_sa = nullptr, *d_st = nullptr, *carry = nullptr; u32 *d_bwt = nullptr; void *SA = nullptr; bool sa64 = false;      // SA: u32 or u64 entries
	size_t free0 = 0, free_min = 0;      // hipMemGetInfo when the builder started / its low-water mark
	std::vector<void *> dead;            // what only the sort needed (ix_release_sort)
	void mark() { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) == hipSuccess) { if (fr < free_min) free_min = fr; } else (void)hipGetLastError(); }
	// the front of the instance's NOMEM message (the caller closes the bracket)
	std::string nomem(const char *who) const { return std::string(who) + (sa64 ? ": hipMalloc (wide builder: 16 bytes per suffix, " : ": hipMalloc (about 52 bytes per suffix, ") + std::to_string((long long)S) + " suffixes"; }
};

// rank[S] = 0 ('$' below every other rank), SA[0] = S ('$' alone), the status words cleared
template <class T> static __global__ void k_ix_init(T *rank, T *SA, u64 *st, i64 S)
{
	if (threadIdx.x == 0 && blockIdx.x == 0) { rank[S] = 0; SA[0] = (T)S; st[0] = 0; st[1] = 0; }
}

// k_index.hip: the geometry, the shared arrays, the upload (ev0, may be null, is recorded behind it), d_bwt and the carries zeroed, the text packed
int ix_begin(gsa_ctx *c, IxBuilt &X, const uint8_t *pac, i64 G, bool sa64, bool samples, hipEvent_t ev0, const char *who);
// the two sorters, from ix_begin's state to the finished SA, primary in X.d_st[1] and their own arrays in X.dead
int ix_sort_narrow(gsa_ctx *c, IxBuilt &X, const char *who);                                    // k_index.hip: u32 SA
int ix_sort_wide(gsa_ctx *c, IxBuilt &X, i64 batch_cap, i64 active_cap, const char *who);      // k_index_wide.hip: u64 SA
static inline i64 ixw_seg(i64 occ_segment) { return occ_segment <= 0 || occ_segment > ((i64)1 << 23) ? (i64)1 << 23 : occ_segment; }      // (2^23 blocks of 128 symbols: totals of 2^30)

#endif
