// gsalign_amd/csrc/k_index.hip -- the BWT/SA half of the index builder on the device (gsa_build_index): what bwa_idx_build does with BWT-SW
// (BWT_Index/bwtindex.c:77-149, bwt.c:101-123) and host/index_io.cpp with SA-IS / a bucket sorter.  The files of the index are fixed by the suffix ORDER
// of T = forward + reverse complement + '$', so any sorter gives the same bytes; this one is prefix doubling on top of the pipeline's radix sort (gsa_sort.hip):
//   first pass   every suffix gets a 63-bit key {its first IX_H0 = 29 bases, 2 bits each, padded with A = 0 | min(bases left, 29)} and all S keys are sorted.
//                END OF TEXT: '$' sorts before A, so a suffix that runs off the end is smaller than a longer one with the same padded prefix.  The five
//                length bits say exactly that -- shorter first -- and no two suffixes shorter than 29 bases share a key, so each of them is a group of its
//                own from here on (a group's members therefore all have h real bases, and at most one of them ends exactly at '$': rank[S] = 0 below).
//                The order never depends on the order the keys went into the sort in.
//   ranks        rank[i] = the first SA slot of the group of suffixes that tie with i so far; SA[0] = S ('$' alone), rank[S] = 0
//   doubling     h = 29, 58, ...: the suffixes whose group still has more than one member (a list that only shrinks) are sorted by
//                {rank[i], rank[i + h]}, their groups split where that key changes, the new ranks written; the host reads ONE counter per round -- the
//                length of the next list -- and stops at 0.  Rounds ~ log2(longest repeat / 29): no depth limit, no fallback.
// From the finished SA plain passes give what derive_bwt_sa and the interleave loop of host/index_io.cpp give: primary, the 2-bit BWT without the '$'
// row, its running counts every 128 symbols (bwt_bwtupdate_core's layout) and the SA samples of every 32nd row.  L2 follows from the closing counts.
#include <chrono>
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

// T, 2 bits per base, 32 bases per word: the forward strand from .pac, behind it its reverse complement (the text gsah_build_index forms), zeros behind that
__global__ void __launch_bounds__(IX_T) k_ix_pack(const uint8_t *__restrict__ pac, i64 G, i64 S, u64 *__restrict__ tw, i64 n_tw)
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

// first-pass keys, two suffixes per thread (S is even): 16-byte key stores, 8-byte value stores
__global__ void __launch_bounds__(IX_T) k_ix_keys0(const u64 *__restrict__ tw, i64 S, u64 *__restrict__ key, u32 *__restrict__ val)
{
	const i64 np = S >> 1;
	for (i64 t = (i64)blockIdx.x * IX_T + threadIdx.x; t < np; t += (i64)gridDim.x * IX_T) {
		const i64 i = 2 * t;
		const i64 l0 = S - i, l1 = l0 - 1;
		ulonglong2 k; uint2 v;
		k.x = ((ix_get32(tw, i) >> 6) << 5) | (u64)(l0 < IX_H0 ? l0 : IX_H0);
		k.y = ((ix_get32(tw, i + 1) >> 6) << 5) | (u64)(l1 < IX_H0 ? l1 : IX_H0);
		v.x = (u32)i; v.y = (u32)(i + 1);
		((ulonglong2 *)key)[t] = k; ((uint2 *)val)[t] = v;
	}
}

// st: [0] length of the next list, [1] primary
__global__ void k_ix_init(u32 *rank, u32 *SA, u32 *st, i64 S)
{
	if (threadIdx.x == 0 && blockIdx.x == 0) { rank[S] = 0; SA[0] = (u32)S; st[0] = 0; st[1] = 0; }
}

// One fused pass over the sorted list of a round (m entries: key, suffix, SA slot; slot = nullptr: entry t sits in slot t + 1, the first pass):
//   component 0  group heads (the key differs from the one in front) -> the group number of every entry, and the slot of every group's head
//   component 1  entries whose group has more than one member -> the next round's list {slot, suffix}, in slot order; its length
struct OpIxRound {
	const u64 *key; const u32 *suf; const u32 *slot; i64 m;
	u32 *grp, *head_slot, *slot_out, *suf_out, *cnt;
	struct Item { u32 head, act, slot, suf; };
	__device__ Item load(i64 t) const
	{
		const u64 k = key[t];
		const bool h = t == 0 || key[t - 1] != k, hn = t + 1 >= m || key[t + 1] != k;
		Item it; it.head = h ? 1u : 0u; it.act = (h && hn) ? 0u : 1u; it.slot = slot ? slot[t] : (u32)(t + 1); it.suf = suf[t];
		return it;
	}
	__device__ i32 value(const Item &it, i64, int c) const { return (i32)(c ? it.act : it.head); }
	__device__ void emit(const Item &it, i64 t, const i32 *v, const i32 *ex) const
	{
		const u32 gi = (u32)(ex[0] + v[0] - 1);
		grp[t] = gi;
		if (it.head) head_slot[gi] = it.slot;
		if (it.act) { slot_out[ex[1]] = it.slot; suf_out[ex[1]] = it.suf; }
	}
	__device__ void done(const i32 *tt) const { *cnt = (u32)tt[1]; }
};

// the round's ranks and SA entries: a suffix's rank is the slot of its group's head; the row that holds suffix 0 is primary (the last round that moves it wins)
__global__ void __launch_bounds__(IX_T) k_ix_apply(i64 m, const u32 *__restrict__ suf, const u32 *__restrict__ slot, const u32 *__restrict__ grp, const u32 *__restrict__ head_slot,
                                                   u32 *__restrict__ rank, u32 *__restrict__ SA, u32 *__restrict__ st)
{
	for (i64 t = (i64)blockIdx.x * IX_T + threadIdx.x; t < m; t += (i64)gridDim.x * IX_T) {
		const u32 s = suf[t], sl = slot ? slot[t] : (u32)(t + 1);
		rank[s] = head_slot[grp[t]];
		SA[sl] = s;
		if (s == 0) st[1] = sl;
	}
}

// keys of a doubling round: {rank[i], rank[i + h]}, b bits each; a suffix that ends within h bases has been alone since the first pass, one that ends
// exactly there reads rank[S] = 0, below every other rank
__global__ void __launch_bounds__(IX_T) k_ix_keys(i64 m, const u32 *__restrict__ suf, const u32 *__restrict__ rank, i64 h, i64 S, int b, u64 *__restrict__ key)
{
	for (i64 t = (i64)blockIdx.x * IX_T + threadIdx.x; t < m; t += (i64)gridDim.x * IX_T) {
		const i64 i = suf[t], j = i + h;
		const u32 r1 = rank[i], r2 = rank[j <= S ? j : S];
		key[t] = ((u64)r1 << b) | (u64)(j <= S ? r2 : 0u);
	}
}

// BWT symbol k comes from row i = k + (k >= primary) (derive_bwt_sa, host/index_io.cpp): T[SA[i] - 1], 16 symbols per word, first symbol in the top bits;
// word kw of the plain BWT is word 16 (kw / 8) + 8 + kw % 8 of the interleaved layout.  One symbol per lane, sixteen lanes OR their bits together.
__global__ void __launch_bounds__(IX_T) k_ix_bwt(i64 S, const u32 *__restrict__ SA, const u64 *__restrict__ tw, const u32 *__restrict__ st, u32 *__restrict__ out)
{
	const i64 primary = (i64)st[1];
	for (i64 base = (i64)blockIdx.x * IX_T; base < S; base += (i64)gridDim.x * IX_T) {      // (base is the same in all lanes of a wave: the shuffles below see full waves)
		const i64 k = base + threadIdx.x;
		u32 v = 0;
		if (k < S) {
			const i64 i = k + (k >= primary ? 1 : 0);
			const i64 p = (i64)SA[i] - 1;
			v = ix_sym(tw, p < 0 ? 0 : p) << ((~(u32)k & 15u) << 1);
		}
		v |= __shfl_xor(v, 1); v |= __shfl_xor(v, 2); v |= __shfl_xor(v, 4); v |= __shfl_xor(v, 8);
		if (k < S && (k & 15) == 0) out[(k >> 7) * 16 + 8 + ((k >> 4) & 7)] = v;
	}
}

// running counts in front of every 128-symbol block (four u64: A, C, G, T), two symbols per pass (sym0, sym0 + 1), and the closing counts behind the last block
struct OpIxOcc {
	u32 *out; i64 S, n_words, k_end; int sym0;
	struct Item { i32 c0, c1; };
	__device__ Item load(i64 g) const
	{
		const uint4 *w4 = (const uint4 *)(out + g * 16 + 8);
		const uint4 a = w4[0], b = w4[1];
		const u32 w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
		const i64 nw = n_words - g * 8, left = S - g * 128;
		i32 cC = 0, cG = 0, cT = 0;
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const u32 x = k < nw ? w[k] : 0u;      // (behind the last word of the last block lie the closing counts)
			const u32 lo = x & 0x55555555u, hi = (x >> 1) & 0x55555555u;
			cT += __popc(lo & hi); cG += __popc(hi & ~lo); cC += __popc(lo & ~hi);
		}
		const i32 cA = (i32)(left < 128 ? left : 128) - cC - cG - cT;      // (the padding of the last word is zeros, not A's)
		Item it;
		if (sym0 == 0) { it.c0 = cA; it.c1 = cC; } else { it.c0 = cG; it.c1 = cT; }
		return it;
	}
	__device__ i32 value(const Item &it, i64, int c) const { return c ? it.c1 : it.c0; }
	__device__ void emit(const Item &, i64 g, const i32 *, const i32 *ex) const
	{
		uint4 o; o.x = (u32)ex[0]; o.y = 0; o.z = (u32)ex[1]; o.w = 0;
		*(uint4 *)(out + g * 16 + 2 * sym0) = o;
	}
	__device__ void done(const i32 *tt) const { u32 *o = out + k_end + 2 * sym0; o[0] = (u32)tt[0]; o[1] = 0; o[2] = (u32)tt[1]; o[3] = 0; }
};

// sa[j] = SA[32 j], sa[0] = -1 (bwt_cal_sa, bwt.c:101-123)
__global__ void __launch_bounds__(IX_T) k_ix_samples(i64 n_sa, const u32 *__restrict__ SA, u64 *__restrict__ sa)
{
	for (i64 j = (i64)blockIdx.x * IX_T + threadIdx.x; j < n_sa; j += (i64)gridDim.x * IX_T) sa[j] = j ? (u64)SA[32 * j] : ~0ull;
}

namespace {
// the builder's device arrays: all freed when the call returns, whichever way
struct IxBufs {
	hipStream_t st; std::vector<void *> p;
	~IxBufs() { (void)hipStreamSynchronize(st); for (void *q : p) (void)hipFree(q); (void)hipGetLastError(); }
	template <class T> bool get(T **out, size_t n) { void *q = nullptr; if (hipMalloc(&q, (n ? n : 1) * sizeof(T) + 256) != hipSuccess) { (void)hipGetLastError(); return false; } p.push_back(q); *out = (T *)q; return true; }
};
}

// pac: host, ceil(G / 4) bytes; primary, L2, bwt[bwt_words], sa[n_sa]: host.  Device bytes per suffix (S = 2G of them): keys 2 x 8, suffixes 2 x 4, slots 2 x 4, rank 4,
// SA 4, the sort's scratch 12 (c->tmp) + its histograms -- 52 bytes, and under 1 byte for the packed text, the BWT words and the samples.
int build_index_device(gsa_ctx *c, const uint8_t *pac, i64 G, u64 *primary, u64 L2[5], u32 *bwt, u64 *sa, double *ms, i32 *rounds)
{
	const i64 S = 2 * G, n = S + 1;
	const i64 n_tw = S / 32 + 3, n_words = (S + 15) / 16, n_blk = (S + 127) / 128, n_bwt = n_words + (n_blk + 1) * 8, n_sa = (S + 32) / 32, k_end = n_blk * 8 + n_words;
	const size_t pac_bytes = (size_t)((G + 3) / 4);
	const int b = ceil_log2_u64((u64)S + 1);      // bits of a rank (0 .. S)
	hipStream_t st = c->stream;
	IxBufs B; B.st = st;
	uint8_t *d_pac; u64 *tw, *keyA, *keyB, *d_sa; u32 *valA, *valB, *slotA, *slotB, *rank, *SA, *d_st, *d_bwt;
	if (!B.get(&d_pac, pac_bytes) || !B.get(&tw, (size_t)n_tw) || !B.get(&keyA, (size_t)n) || !B.get(&keyB, (size_t)n) || !B.get(&valA, (size_t)n) || !B.get(&valB, (size_t)n) ||
	    !B.get(&slotA, (size_t)n) || !B.get(&slotB, (size_t)n) || !B.get(&rank, (size_t)n + 1) || !B.get(&SA, (size_t)n + 32) || !B.get(&d_st, (size_t)8) ||
	    !B.get(&d_bwt, (size_t)n_bwt + 16) || !B.get(&d_sa, (size_t)n_sa))
		return gsa_fail(c, GSA_ERR_NOMEM, "gsa_build_index: hipMalloc (about 52 bytes per suffix, " + std::to_string((long long)S) + " suffixes)");
	hipEvent_t ev[2] = { nullptr, nullptr };
	struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int k = 0; k < 2; k++) if (e[k]) (void)hipEventDestroy(e[k]); } } evg{ ev };
	GSA_CHECK(c, hipEventCreate(&ev[0])); GSA_CHECK(c, hipEventCreate(&ev[1]));
	GSA_CHECK(c, hipMemcpyAsync(d_pac, pac, pac_bytes, hipMemcpyHostToDevice, st));
	GSA_CHECK(c, hipEventRecord(ev[0], st));
	GSA_CHECK(c, hipMemsetAsync(d_bwt, 0, ((size_t)n_bwt + 16) * 4, st));
	hipLaunchKernelGGL(k_ix_init, dim3(1), dim3(64), 0, st, rank, SA, d_st, S);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_ix_pack, dim3(ix_grid(n_tw)), dim3(IX_T), 0, st, (const uint8_t *)d_pac, G, S, tw, n_tw);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_ix_keys0, dim3(ix_grid(S / 2)), dim3(IX_T), 0, st, (const u64 *)tw, S, keyA, valA);
	GSA_CHECK(c, hipGetLastError());
	if (int rc = gsa_sort_pairs_u64_u32(c, keyA, keyB, valA, valB, (size_t)S, 0, 2 * IX_H0 + 5)) return rc;
	// the group numbers and the head slots of a round live where the sort's input keys were (dead once sorted): m + m words
	u32 *grp = (u32 *)keyA, *head_slot = grp + n;
	const u32 *slot = nullptr; u32 *slot_out = slotA;
	i64 m = S, h = IX_H0; i32 nr = 0;
	for (;;) {
		OpIxRound op = { keyB, valB, slot, m, grp, head_slot, slot_out, valA, d_st };
		if (int rc = lb_launch<2>(c, m, op, st)) return rc;
		hipLaunchKernelGGL(k_ix_apply, dim3(ix_grid(m)), dim3(IX_T), 0, st, m, (const u32 *)valB, slot, (const u32 *)grp, (const u32 *)head_slot, rank, SA, d_st);
		GSA_CHECK(c, hipGetLastError());
		u32 left = 0;
		GSA_CHECK(c, hipMemcpyAsync(&left, d_st, 4, hipMemcpyDeviceToHost, st));
		GSA_CHECK(c, hipStreamSynchronize(st));
		if (left == 0) break;
		if (++nr > 64) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_build_index: the suffix groups do not resolve");
		m = (i64)left;
		hipLaunchKernelGGL(k_ix_keys, dim3(ix_grid(m)), dim3(IX_T), 0, st, m, (const u32 *)valA, (const u32 *)rank, h, S, b, keyA);
		GSA_CHECK(c, hipGetLastError());
		if (int rc = gsa_sort_pairs_u64_u32(c, keyA, keyB, valA, valB, (size_t)m, 0, 2 * b)) return rc;
		slot = slot_out; slot_out = slot_out == slotA ? slotB : slotA;
		h *= 2;
	}
	hipLaunchKernelGGL(k_ix_bwt, dim3(ix_grid(S)), dim3(IX_T), 0, st, S, (const u32 *)SA, (const u64 *)tw, (const u32 *)d_st, d_bwt);
	GSA_CHECK(c, hipGetLastError());
	for (int sym0 = 0; sym0 < 4; sym0 += 2) { OpIxOcc op = { d_bwt, S, n_words, k_end, sym0 }; if (int rc = lb_launch<2>(c, n_blk, op, st)) return rc; }
	hipLaunchKernelGGL(k_ix_samples, dim3(ix_grid(n_sa)), dim3(IX_T), 0, st, n_sa, (const u32 *)SA, d_sa);
	GSA_CHECK(c, hipGetLastError());
	GSA_CHECK(c, hipEventRecord(ev[1], st));
	u32 h_st[2] = { 0, 0 }; i32 lberr = 0;
	GSA_CHECK(c, hipMemcpyAsync(h_st, d_st, 8, hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipMemcpyAsync(&lberr, c->d_mail.as<i32>() + M_LBERR, 4, hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipMemcpyAsync(bwt, d_bwt, (size_t)n_bwt * 4, hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipMemcpyAsync(sa, d_sa, (size_t)n_sa * 8, hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipStreamSynchronize(st));
	if (lberr) return gsa_fail(c, GSA_ERR_STATE, "internal: look-back scan timed out");
	float fms = 0; if (hipEventElapsedTime(&fms, ev[0], ev[1]) != hipSuccess) { fms = 0; (void)hipGetLastError(); }
	*primary = (u64)h_st[1];
	L2[0] = 0;
	for (int k = 0; k < 4; k++) L2[k + 1] = L2[k] + ((u64)bwt[k_end + 2 * k] | ((u64)bwt[k_end + 2 * k + 1] << 32));
	if (L2[4] != (u64)S) return gsa_fail(c, GSA_ERR_STATE, "internal: gsa_build_index: the symbol counts do not add up");
	*ms = (double)fms; *rounds = nr;
	return GSA_OK;
}
