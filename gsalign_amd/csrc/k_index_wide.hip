// gsalign_amd/csrc/k_index_wide.hip -- the wide instance of the device index builder (gsa_build_index_opts, GSA_CREATE_SORT_WIDE): k_index.hip's prefix doubling for
// texts of more than 2^31 - 2 suffixes.  Suffix numbers, ranks and SA slots are 64-bit; the radix sort (gsa_sort.hip) and the fused scans (gsa_scan.h) stay as they
// are, 32-bit, because no call of either ever sees more than 2^31 - 2 elements: the suffixes are worked on in BATCHES.
//   batches      a batch is a range of classes of the first IXW_P = 8 bases, i.e. of the top 16 bits of the first-pass key: equal keys share a batch, and since the
//                rounds only refine the first-pass order a group never crosses a batch boundary.  k_ixw_hist counts the classes (64-bit counters), the host cuts the
//                histogram into consecutive ranges of at most batch_cap suffixes (gsa_plan_index_batches); batch b owns the SA slots [base_b, base_b + count_b).
//   first pass   per batch: its suffix positions in text order (OpIxwPick, a fused pass over all S positions), their 63-bit keys, the sort with the list index as
//                the value, a gather that puts the 64-bit positions into sorted order.  The 33-bit suffix number is never a sort value.
//   doubling     rounds are global (h is the same for all batches), batches run one after the other inside a round: the batch's part of the active list is sorted by
//                {rank[i] - base_b, rank[i + h]} (31 + 33 bits at most), gathered, split (OpIxwRound) and applied (k_ixw_apply).  A later batch of the round may read
//                rank[i + h] of a suffix an earlier batch has refined in this very round: that rank is finer and order-consistent, which is all the key needs
//                (the argument is in DESIGN.md section 8d.1).  Slots travel relative to the batch base, in 32 bits.
// This file is the sorter only (ix_sort_wide, between ix_begin and the derivation half: both in k_index.hip, the latter instantiated for the 64-bit SA, its Occ running
// counts scanned in segments of occ_segment blocks whose totals fit the scan's i32) and the batch planner.
#include <chrono>
#include "gsa_index.h"

#define IXW_P 8
#define IXW_NCLS (1 << (2 * IXW_P))
#define IXW_LIMIT (((i64)1 << 31) - 2)      // elements of one sort / one fused scan

__device__ __forceinline__ u32 ixw_class(const u64 *__restrict__ tw, i64 i) { return (u32)(ix_get32(tw, i) >> (64 - 2 * IXW_P)); }

// class counts: a thread takes the 32 positions of one text word and adds a run of equal classes at once (a homopolymer run is one atomic per word, not 32)
__global__ void __launch_bounds__(IX_T) k_ixw_hist(const u64 *__restrict__ tw, i64 S, unsigned long long *hist)
{
	const i64 nw = (S + 31) >> 5;
	for (i64 w = (i64)blockIdx.x * IX_T + threadIdx.x; w < nw; w += (i64)gridDim.x * IX_T) {
		const u64 a = tw[w], b = tw[w + 1];
		u32 prev = 0, run = 0;
		for (int k = 0; k < 32; k++) {
			if (w * 32 + k >= S) break;
			const u64 x = k ? (a << (2 * k)) | (b >> (64 - 2 * k)) : a;
			const u32 cls = (u32)(x >> (64 - 2 * IXW_P));
			if (run && cls == prev) { run++; continue; }
			if (run) atomicAdd(&hist[prev], (unsigned long long)run);
			prev = cls; run = 1;
		}
		if (run) atomicAdd(&hist[prev], (unsigned long long)run);
	}
}

// the positions of a batch's suffixes, in text order (classes c0 .. c1 - 1; the count is the histogram's, at most 2^31 - 2)
struct OpIxwPick {
	const u64 *tw; u32 c0, c1; u64 *pos; i64 room;
	struct Item { u32 in; };
	__device__ Item load(i64 i) const { const u32 cl = ixw_class(tw, i); Item it; it.in = (cl >= c0 && cl < c1) ? 1u : 0u; return it; }
	__device__ i32 value(const Item &it, i64, int) const { return (i32)it.in; }
	__device__ void emit(const Item &it, i64 i, const i32 *, const i32 *ex) const { if (it.in && (i64)ex[0] < room) pos[ex[0]] = (u64)i; }
	__device__ void done(const i32 *) const {}
};

__global__ void __launch_bounds__(IX_T) k_ixw_keys0(i64 m, const u64 *__restrict__ pos, const u64 *__restrict__ tw, i64 S, u64 *__restrict__ key, u32 *__restrict__ val)
{
	for (i64 t = (i64)blockIdx.x * IX_T + threadIdx.x; t < m; t += (i64)gridDim.x * IX_T) { key[t] = ix_key0(tw, (i64)pos[t], S); val[t] = (u32)t; }
}

// the sorted list's suffixes from the sort's values (indices into the unsorted list)
__global__ void __launch_bounds__(IX_T) k_ixw_gather(i64 m, const u64 *__restrict__ src, const u32 *__restrict__ idx, u64 *__restrict__ dst)
{
	for (i64 t = (i64)blockIdx.x * IX_T + threadIdx.x; t < m; t += (i64)gridDim.x * IX_T) dst[t] = src[idx[t]];
}

// OpIxRound (k_index.hip) for one batch: slots are relative to the batch base (slot = nullptr: entry t sits in slot t, the first pass), suffixes 64-bit.  The next
// round's entries go behind those of the batches in front: *off_in is where (the sum of their counts, written by THEIR passes: same stream, no host read in between),
// off_in[1] gets this batch's end.  The list holds `cap` entries: what does not fit is counted, not written, and the host sees the sum when it reads the offsets.
struct OpIxwRound {
	const u64 *key; const u64 *suf; const u32 *slot; i64 m;
	u32 *grp, *head_slot, *slot_out; u64 *suf_out; i64 cap; u64 *off_in;
	struct Item { u32 head, act, slot, pad; u64 suf; };
	__device__ Item load(i64 t) const
	{
		const u64 k = key[t];
		const bool h = t == 0 || key[t - 1] != k, hn = t + 1 >= m || key[t + 1] != k;
		Item it; it.head = h ? 1u : 0u; it.act = (h && hn) ? 0u : 1u; it.slot = slot ? slot[t] : (u32)t; it.pad = 0; it.suf = suf[t];
		return it;
	}
	__device__ i32 value(const Item &it, i64, int c) const { return (i32)(c ? it.act : it.head); }
	__device__ void emit(const Item &it, i64 t, const i32 *v, const i32 *ex) const
	{
		const u32 gi = (u32)(ex[0] + v[0] - 1);
		grp[t] = gi;
		if (it.head) head_slot[gi] = it.slot;
		if (it.act) { const u64 o = off_in[0] + (u64)(u32)ex[1]; if (o < (u64)cap) { slot_out[o] = it.slot; suf_out[o] = it.suf; } }
	}
	__device__ void done(const i32 *tt) const { off_in[1] = off_in[0] + (u64)(u32)tt[1]; }
};

// k_ix_apply for one batch: base + the relative slots
__global__ void __launch_bounds__(IX_T) k_ixw_apply(i64 m, const u64 *__restrict__ suf, const u32 *__restrict__ slot, const u32 *__restrict__ grp, const u32 *__restrict__ head_slot, u64 base,
                                                    u64 *__restrict__ rank, u64 *__restrict__ SA, u64 *__restrict__ st)
{
	for (i64 t = (i64)blockIdx.x * IX_T + threadIdx.x; t < m; t += (i64)gridDim.x * IX_T) {
		const u64 s = suf[t], sl = base + (slot ? slot[t] : (u32)t);
		rank[s] = base + head_slot[grp[t]];
		SA[sl] = s;
		if (s == 0) st[1] = sl;
	}
}

// keys of a doubling round for one batch: {rank[i] - base, rank[i + h]}, the second b bits wide; val = the entry's index in the batch's list
__global__ void __launch_bounds__(IX_T) k_ixw_keys(i64 m, const u64 *__restrict__ suf, const u64 *__restrict__ rank, i64 h, i64 S, u64 base, int b, u64 *__restrict__ key, u32 *__restrict__ val)
{
	for (i64 t = (i64)blockIdx.x * IX_T + threadIdx.x; t < m; t += (i64)gridDim.x * IX_T) {
		const i64 i = (i64)suf[t], j = i + h;
		const u64 r1 = rank[i] - base, r2 = rank[j <= S ? j : S];
		key[t] = (r1 << b) | (j <= S ? r2 : 0ull);
		val[t] = (u32)t;
	}
}

// ---- the batch planner (host) --------------------------------------------------------------------------------------------------------------------------------
// hist[n_classes] -> consecutive class ranges of at most batch_cap suffixes each.  first[b] = the first class of batch b, first[*n_batches] = n_classes;
// base[b] = 1 + the suffixes in front of batch b ('$' keeps slot 0), base[*n_batches] = 1 + all of them.  A class larger than the cap is a batch of its own: empty
// classes between two such classes are a batch of no suffix, which the builder skips.  first / base hold max_batches + 1 entries.
extern "C" int gsa_plan_index_batches(const uint64_t *hist, int64_t n_classes, int64_t batch_cap, int64_t max_batches, int64_t *first, uint64_t *base, int64_t *n_batches)
{
	if (!hist || !first || !base || !n_batches || n_classes <= 0 || batch_cap <= 0 || max_batches <= 0) return gsa_fail(nullptr, GSA_ERR_ARG, "gsa_plan_index_batches: bad argument");
	i64 nb = 0, start = 0; u64 cnt = 0, tot = 0;
	for (i64 c = 0; c < n_classes; c++) {
		const u64 h = hist[c];
		if (h > (u64)IXW_LIMIT) {
			std::string name;
			int P = 0; while (((i64)1 << (2 * P)) < n_classes) P++;
			if (((i64)1 << (2 * P)) == n_classes) { name = " ("; for (int k = P - 1; k >= 0; k--) name += "ACGT"[(c >> (2 * k)) & 3]; name += ")"; }
			return gsa_fail(nullptr, GSA_ERR_LIMIT, "the index builder's batches: prefix class " + std::to_string((long long)c) + name + " holds " + std::to_string((unsigned long long)h) +
			                " suffixes, more than the 2 147 483 646 one sort takes");
		}
		if (c > start && cnt + h > (u64)batch_cap) {
			if (nb >= max_batches) return gsa_fail(nullptr, GSA_ERR_ARG, "gsa_plan_index_batches: more batches than max_batches");
			first[nb] = start; base[nb] = 1 + tot; nb++; tot += cnt; start = c; cnt = 0;
		}
		cnt += h;
	}
	if (nb >= max_batches) return gsa_fail(nullptr, GSA_ERR_ARG, "gsa_plan_index_batches: more batches than max_batches");
	first[nb] = start; base[nb] = 1 + tot; nb++; tot += cnt;
	first[nb] = n_classes; base[nb] = 1 + tot;
	*n_batches = nb;
	return GSA_OK;
}

static i64 ixw_cap(i64 batch_cap) { return batch_cap <= 0 ? (i64)1 << 30 : (batch_cap > IXW_LIMIT ? IXW_LIMIT : batch_cap); }

// From ix_begin's state (k_index.hip) to the finished 64-bit SA; X.batches: those that hold a suffix, X.dead: everything only the rounds needed.
// Device bytes: 16 per suffix (rank, SA), 52 per entry of the largest batch (unsorted positions 8, keys 2 x 8, values 2 x 4, sorted positions 8, the sort's scratch 12 and
// its histograms; the group numbers and head slots of a round live where the sort's input keys were), 24 per entry of the active list (relative slot 4, suffix 8, twice), under
// 1 per suffix for the packed text, the BWT words and the samples.
int ix_sort_wide(gsa_ctx *c, IxBuilt &X, i64 batch_cap, i64 active_cap, const char *who)
{
	const i64 S = X.S;
	const int b = ceil_log2_u64((u64)S + 1);      // bits of a rank (0 .. S)
	batch_cap = ixw_cap(batch_cap);
	hipStream_t st = c->stream;
	IxBufs &B = X.B;
	const std::string nomem = X.nomem(who);
	const u64 *tw = X.tw; u64 *rank, *SA = (u64 *)X.SA, *d_st = X.d_st; unsigned long long *d_hist;
	if (!B.get(&rank, (size_t)X.n + 1) || !B.get(&d_hist, (size_t)IXW_NCLS)) return gsa_fail(c, GSA_ERR_NOMEM, nomem + ")");
	GSA_CHECK(c, hipMemsetAsync(d_hist, 0, (size_t)IXW_NCLS * 8, st));
	hipLaunchKernelGGL(k_ix_init<u64>, dim3(1), dim3(64), 0, st, rank, SA, d_st, S);
	GSA_CHECK(c, hipGetLastError());
	hipLaunchKernelGGL(k_ixw_hist, dim3(ix_grid((S + 31) / 32)), dim3(IX_T), 0, st, tw, S, d_hist);
	GSA_CHECK(c, hipGetLastError());
	std::vector<uint64_t> hist((size_t)IXW_NCLS), base((size_t)IXW_NCLS + 1); std::vector<int64_t> first((size_t)IXW_NCLS + 1);
	GSA_CHECK(c, hipMemcpyAsync(hist.data(), d_hist, (size_t)IXW_NCLS * 8, hipMemcpyDeviceToHost, st));
	GSA_CHECK(c, hipStreamSynchronize(st));
	int64_t nb = 0;
	if (int rc = gsa_plan_index_batches(hist.data(), IXW_NCLS, batch_cap, IXW_NCLS, first.data(), base.data(), &nb)) return gsa_fail(c, rc, std::string(who) + ": " + gsa_last_error(nullptr));
	if (base[(size_t)nb] != (u64)S + 1) return gsa_fail(c, GSA_ERR_STATE, std::string("internal: ") + who + ": the prefix classes do not add up");
	i64 mb = 0, used = 0;
	for (i64 k = 0; k < nb; k++) { const i64 cn = (i64)(base[(size_t)k + 1] - base[(size_t)k]); if (cn > mb) mb = cn; if (cn > 0) used++; }
	X.batches = used;
	// the batch arrays, then the active lists in what is left (at most S entries: every suffix still tied after the first pass)
	u64 *pos, *keyA, *keyB, *sufS; u32 *valA, *valB;
	if (!B.get(&pos, (size_t)mb) || !B.get(&keyA, (size_t)mb + 1) || !B.get(&keyB, (size_t)mb) || !B.get(&sufS, (size_t)mb) || !B.get(&valA, (size_t)mb) || !B.get(&valB, (size_t)mb))
		return gsa_fail(c, GSA_ERR_NOMEM, nomem + ", 52 per entry of a batch of " + std::to_string((long long)mb) + ")");
	i64 a_cap = S;
	{
		size_t fr = 0, tot = 0;
		if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = ~(size_t)0; }
		// still to come: the sort's scratch (12 bytes per entry of the largest batch, its histograms, the quarter gsa_sort adds: 15.6, taken as 18), the scans' status words, 1 GB
		const size_t later = (size_t)mb * 18 + (size_t)(S / 2048) * 16 + ((size_t)1 << 30);
		const i64 fit = fr > later ? (i64)((fr - later) / 24) : 0;
		if (fit < a_cap) a_cap = fit;
	}
	if (active_cap > 0 && active_cap < a_cap) a_cap = active_cap;      // (gsa_set_index_build_caps: the test hook for a list that does not fit)
	u32 *slotL[2]; u64 *sufL[2], *d_off;
	if (a_cap < 1 || !B.get(&slotL[0], (size_t)a_cap) || !B.get(&slotL[1], (size_t)a_cap) || !B.get(&sufL[0], (size_t)a_cap) || !B.get(&sufL[1], (size_t)a_cap) || !B.get(&d_off, (size_t)nb + 2))
		return gsa_fail(c, GSA_ERR_NOMEM, nomem + ", 24 per entry of an active list of " + std::to_string((long long)a_cap) + ")");
	X.mark();
	u32 *grp = (u32 *)keyA, *head_slot = grp + mb;      // (where the sort's input keys were: dead once sorted)
	std::vector<i64> off[2], cnt[2], done_k; std::vector<u64> h_off((size_t)nb + 2);
	for (int k = 0; k < 2; k++) { off[k].assign((size_t)nb, 0); cnt[k].assign((size_t)nb, 0); }
	// one batch of one round, from the sorted keys in keyB / the sort's values in valB on: gather, split, apply.  The j-th batch a round works on appends its
	// next list at d_off[j] and leaves d_off[j + 1]; nothing is read home between the batches
	auto finish_batch = [&](i64 k, i64 m, const u64 *src, const u32 *slot_in, int nxt) -> int {
		hipLaunchKernelGGL(k_ixw_gather, dim3(ix_grid(m)), dim3(IX_T), 0, st, m, src, (const u32 *)valB, sufS);
		GSA_CHECK(c, hipGetLastError());
		OpIxwRound op = { keyB, sufS, slot_in, m, grp, head_slot, slotL[nxt], sufL[nxt], a_cap, d_off + done_k.size() };
		if (int rc = lb_launch<2>(c, m, op, st)) return rc;
		hipLaunchKernelGGL(k_ixw_apply, dim3(ix_grid(m)), dim3(IX_T), 0, st, m, (const u64 *)sufS, slot_in, (const u32 *)grp, (const u32 *)head_slot, (u64)base[(size_t)k], rank, SA, d_st);
		GSA_CHECK(c, hipGetLastError());
		done_k.push_back(k);
		return GSA_OK;
	};
	// the round's ONE read-back: where every batch's next list begins and ends; the length of the whole list
	auto end_round = [&](int nxt, i64 &next_len) -> int {
		const size_t J = done_k.size();
		GSA_CHECK(c, hipMemcpyAsync(h_off.data(), d_off, (J + 1) * 8, hipMemcpyDeviceToHost, st));
		GSA_CHECK(c, hipStreamSynchronize(st));
		for (size_t k = 0; k < (size_t)nb; k++) cnt[nxt][k] = 0;
		for (size_t j = 0; j < J; j++) { off[nxt][(size_t)done_k[j]] = (i64)h_off[j]; cnt[nxt][(size_t)done_k[j]] = (i64)(h_off[j + 1] - h_off[j]); }
		next_len = (i64)h_off[J];
		done_k.clear();
		if (next_len > a_cap)
			return gsa_fail(c, GSA_ERR_NOMEM, std::string(who) + ": the list of suffixes that still tie needs " + std::to_string((long long)next_len) + " entries of 24 bytes, there is room for " +
			                std::to_string((long long)a_cap) + " beside " + std::to_string((long long)S) + " suffixes of 16 bytes and a batch of " + std::to_string((long long)mb));
		return GSA_OK;
	};
	i64 next_len = 0;
	GSA_CHECK(c, hipMemsetAsync(d_off, 0, 8, st));
	for (i64 k = 0; k < nb; k++) {
		const i64 m = (i64)(base[(size_t)k + 1] - base[(size_t)k]);
		if (m == 0) continue;
		OpIxwPick pick = { tw, (u32)first[(size_t)k], (u32)first[(size_t)k + 1], pos, m };
		if (int rc = lb_launch<1>(c, S, pick, st)) return rc;
		hipLaunchKernelGGL(k_ixw_keys0, dim3(ix_grid(m)), dim3(IX_T), 0, st, m, (const u64 *)pos, (const u64 *)tw, S, keyA, valA);
		GSA_CHECK(c, hipGetLastError());
		if (int rc = gsa_sort_pairs_u64_u32(c, keyA, keyB, valA, valB, (size_t)m, 0, 2 * IX_H0 + 5)) return rc;
		X.mark();
		if (int rc = finish_batch(k, m, pos, nullptr, 0)) return rc;
	}
	if (int rc = end_round(0, next_len)) return rc;
	X.active = next_len;
	i64 h = IX_H0; i32 nr = 0; int cur = 0;
	while (next_len > 0) {
		if (++nr > 64) return gsa_fail(c, GSA_ERR_STATE, std::string("internal: ") + who + ": the suffix groups do not resolve");
		const int nxt = cur ^ 1;
		for (i64 k = 0; k < nb; k++) {
			const i64 m = cnt[cur][(size_t)k], o = off[cur][(size_t)k];
			if (m == 0) continue;
			const int bb = ceil_log2_u64(base[(size_t)k + 1] - base[(size_t)k] + 1);      // bits of a rank relative to the batch base
			hipLaunchKernelGGL(k_ixw_keys, dim3(ix_grid(m)), dim3(IX_T), 0, st, m, (const u64 *)(sufL[cur] + o), (const u64 *)rank, h, S, (u64)base[(size_t)k], b, keyA, valA);
			GSA_CHECK(c, hipGetLastError());
			if (int rc = gsa_sort_pairs_u64_u32(c, keyA, keyB, valA, valB, (size_t)m, 0, b + bb)) return rc;
			if (int rc = finish_batch(k, m, sufL[cur] + o, slotL[cur] + o, nxt)) return rc;
		}
		if (int rc = end_round(nxt, next_len)) return rc;
		cur = nxt; h *= 2;
	}
	X.mark();
	X.rounds = nr;
	X.dead = { (void *)rank, (void *)d_hist, (void *)pos, (void *)keyA, (void *)keyB, (void *)sufS, (void *)valA, (void *)valB, (void *)slotL[0], (void *)slotL[1], (void *)sufL[0], (void *)sufL[1], (void *)d_off };
	return GSA_OK;
}
