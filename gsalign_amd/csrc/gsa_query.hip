// gsalign_amd/csrc/gsa_query.hip -- how a query reaches the device: the Uploader's thread, the two query slots and their prefetch, gsa_set_query*, a bundle's tables
#include <cstring>
#include "gsa_ctx.h"

void Uploader::run()
{
	(void)hipSetDevice(device);
	for (;;) {
		Job j;
		{ std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return stop || !q.empty(); }); if (q.empty()) return; j = std::move(q.front()); q.pop_front(); if (n_demand > 0) n_demand--; }
		const auto t0 = std::chrono::steady_clock::now();
		// a failed copy (a host pointer the runtime cannot read, a device fault) must not look like an upload: the slot keeps the first error
		// and the align call that adopts the slot fails with GSA_ERR_HIP (slot_finish)
		hipError_t e_first = hipSuccess;
		for (const Piece &p : j.pieces) if (p.n) { const hipError_t e = hipMemcpyAsync(p.dst, p.src, p.n, hipMemcpyHostToDevice, st); if (e != hipSuccess && e_first == hipSuccess) e_first = e; bytes += p.n; }
		{ const hipError_t e = hipStreamSynchronize(st); if (e != hipSuccess && e_first == hipSuccess) e_first = e; }
		(void)hipGetLastError();
		if (e_first != hipSuccess && j.err) { int none = 0; j.err->compare_exchange_strong(none, (int)e_first); }
		const auto t1 = std::chrono::steady_clock::now();
		{ std::lock_guard<std::mutex> g(mu); copy_ms += std::chrono::duration<double, std::milli>(t1 - t0).count(); wait_ms += std::chrono::duration<double, std::milli>(t0 - j.t_push).count(); jobs++; }
		j.busy->fetch_sub(1, std::memory_order_release);
	}
}

// A context needs this slot NOW: its upload, if it has not started, goes to the front of the queue (uploads somebody waits for before
// uploads of contigs whose turn comes later: at the start of a run every context has two contigs in the queue and the GPU has nothing)
static void slot_demand(gsa_ctx *c, QuerySlot &s)
{
	if (s.busy.load(std::memory_order_acquire) > 0 && c->up) {
		Uploader *u = c->up;
		std::lock_guard<std::mutex> g(u->mu);
		for (size_t k = u->n_demand; k < u->q.size(); k++) if (u->q[k].busy == &s.busy) {
			Uploader::Job j = std::move(u->q[k]); u->q.erase(u->q.begin() + (long)k); u->q.insert(u->q.begin() + (long)u->n_demand, std::move(j)); u->n_demand++;
			break;
		}
	}
	slot_wait(s);
}

// Back to stage 0: nothing of the previous run may still be in flight or half-consumed (the early striped DP launch
// writes e_* buffers the next stage 2 would reuse).
int reset_run_state(gsa_ctx *c)
{
	if (c->early_in_flight) { GSA_CHECK(c, hipStreamSynchronize(c->stream_aux[0])); c->early_in_flight = false; }
	c->n_early = 0; c->early_listed = false; c->early_consumed = false;
	c->stage = 0; c->split = false; c->b_lists.clear();
	c->n_seeds = 0; c->n_groups = 0; c->n_blocks2 = 0; c->blocks.clear(); c->frags_stage = 0; c->have_host_seeds = false; c->ev_pending = 0; c->s2_host = false;
	memset(c->counters, 0, sizeof(c->counters)); memset(c->kernel_ms, 0, sizeof(c->kernel_ms));
	return GSA_OK;
}

// the 64-bit seed key (PosDiff, position) of a query of `tot` bases with `pd_span` PosDiff values; `what`: "contig" / "bundle", for the message
static int seed_key_geometry(gsa_ctx *c, i64 tot, i64 pd_span, const char *what)
{
	c->qlen = (i32)tot; c->pd_span = pd_span;
	c->qbits = ceil_log2_u64((u64)tot + 1); if (c->qbits < 1) c->qbits = 1;
	c->pdbits = ceil_log2_u64((u64)pd_span);
	if (c->qbits + c->pdbits > 64) return gsa_fail(c, GSA_ERR_LIMIT, std::string(what) + " too long for the 64-bit seed key");
	return GSA_OK;
}
static int query_geometry(gsa_ctx *c, int32_t qlen)      // one contig
{
	c->bnd.n = 0; c->bnd.lmax = qlen; c->bnd.pds = 0; c->bnd.off = (const i32 *)c->d_zero.p; c->bnd.chunk_contig = (const uint16_t *)c->d_zero.p;      // (contig 0 at offset 0: readable without asking bnd.n)
	return seed_key_geometry(c, qlen, 2 * c->G + (i64)qlen + 2, "contig");
}

// is p device memory of this context's GPU?  (a host pointer handed to a kernel would be a GPU fault, not an error code)
static bool device_ptr_of(const gsa_ctx *c, const void *p)
{
	hipPointerAttribute_t at;
	if (p && hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == c->device) return true;
	(void)hipGetLastError();
	return false;
}

// ---- query slots (QuerySlot, gsa_ctx.h) ----
// a slot's buffer grows: nothing may still read or write it (the stages of the contig it held are over -- the API is synchronous --
// but an upload may be on its way)
static void *slot_ensure_bytes(gsa_ctx *c, DevBuf &b, size_t bytes, bool pinned)
{
	if (bytes && bytes <= b.cap) return b.p;
	return pinned ? (void *)pin_ensure<uint8_t>(c, b, bytes) : (void *)dev_ensure<uint8_t>(c, b, bytes);
}

// the slot for a contig that no prefetch brought: the current one unless a prefetched contig waits there (-1: one waits in both)
static int slot_pick_free(const gsa_ctx *c)
{
	int i = (c->q_cur == 1 && !c->qs[1].pending) ? 1 : 0;
	if (c->qs[i].pending) i ^= 1;
	return c->qs[i].pending ? -1 : i;
}

// The concatenation of a bundle in slot s -- every contig starts on a chunk edge, as it does alone -- and its tables in pinned staging: off[n + 1] (i32) |
// chunk_contig[n_chunks] (u16) | n source entries of src_entry_bytes each, which the caller fills at o_src.  *t_bytes: the size of the tables.
static int slot_tables(gsa_ctx *c, QuerySlot &s, const char *const *query, const int32_t *qlen, int32_t n, size_t src_entry_bytes, size_t *t_bytes)
{
	s.b_off.assign((size_t)n + 1, 0); s.b_qlen.assign(qlen, qlen + n); s.src.assign(query, query + n);
	i64 tot = 0; i32 lmax = 0;
	for (int k = 0; k < n; k++) {
		if (qlen[k] < 0 || (qlen[k] > 0 && !query[k])) return GSA_ERR_ARG;
		s.b_off[(size_t)k] = (i32)tot;
		tot += ((i64)qlen[k] + GSA_CHUNK - 1) / GSA_CHUNK * GSA_CHUNK;
		if (tot >= (1ll << 31) - 2 * GSA_CHUNK) return gsa_fail(c, GSA_ERR_LIMIT, "bundle longer than 2^31 bases");
		if (qlen[k] > lmax) lmax = qlen[k];
	}
	s.b_off[(size_t)n] = (i32)tot; s.tot = tot; s.lmax = lmax; s.n = n;
	const i64 n_chunks = s.tot / GSA_CHUNK;
	s.o_cc = ((size_t)n + 1) * 4; s.o_src = (s.o_cc + (size_t)n_chunks * 2 + 15) & ~(size_t)15;
	*t_bytes = s.o_src + (size_t)n * src_entry_bytes;
	if (!slot_ensure_bytes(c, s.p_bndtab, *t_bytes + 16, true) || !slot_ensure_bytes(c, s.d_bndtab, *t_bytes + 16, false) || !slot_ensure_bytes(c, s.d_query, (size_t)s.tot + 64, false)) return GSA_ERR_NOMEM;
	uint8_t *ht = s.p_bndtab.as<uint8_t>();
	memcpy(ht, s.b_off.data(), s.o_cc);
	uint16_t *cc = (uint16_t *)(ht + s.o_cc);
	for (int k = 0; k < n; k++) for (i64 ch = s.b_off[(size_t)k] / GSA_CHUNK; ch < s.b_off[(size_t)k + 1] / GSA_CHUNK; ch++) cc[ch] = (uint16_t)k;
	return GSA_OK;
}

// the tail of every contig of a bundle up to its chunk edge reads 'N' (a match stops there exactly as it stops at the end of a sequence)
extern "C" __global__ void __launch_bounds__(256) k_bundle_pad(const i32 *__restrict__ off, const i32 *__restrict__ len, uint8_t *dst)
{
	const i32 k = blockIdx.x; const i64 b = (i64)off[k] + len[k], e = off[k + 1];
	for (i64 t = b + threadIdx.x; t < e; t += 256) dst[t] = (uint8_t)'N';
}
// The concatenation of device-resident contigs: one workgroup per chunk copies its 10 000 bytes (or the tail of its contig and 'N's).
struct BundleSrc { const uint8_t *p; i32 len, _pad; };
extern "C" __global__ void __launch_bounds__(256) k_bundle_gather(const i32 *__restrict__ off, const uint16_t *__restrict__ chunk_contig, const BundleSrc *__restrict__ src, uint8_t *dst)
{
	const i32 chunk = blockIdx.x, ci = chunk_contig[chunk];
	const i64 g0 = (i64)chunk * GSA_CHUNK; const i32 l0 = (i32)(g0 - off[ci]);
	const BundleSrc sc = src[ci];
	const i32 have = sc.len - l0 < GSA_CHUNK ? sc.len - l0 : GSA_CHUNK;
	for (i32 t = threadIdx.x; t < GSA_CHUNK; t += 256) dst[g0 + t] = t < have ? sc.p[l0 + t] : (uint8_t)'N';
}

// Hands the Uploader the copies that fill slot `s` from host memory: one contig (n = 0, query[0] / qlen[0]) or the concatenation of a
// bundle + its tables (the 'N' tails are written by slot_finish on the main stream: nothing but copies on the upload stream).
static int slot_upload(gsa_ctx *c, QuerySlot &s, const char *const *query, const int32_t *qlen, int32_t n)
{
	slot_wait(s);      // (a cancelled upload into this slot may still be on its way)
	s.up_err.store(0);      // (... and whatever became of it no longer matters)
	Uploader::Job job; job.busy = &s.busy; job.err = &s.up_err;
	if (n == 0) {
		s.n = 0; s.tot = qlen[0]; s.lmax = qlen[0]; s.src.assign(1, query[0]); s.b_qlen.assign(1, qlen[0]); s.b_off.clear();
		if (!slot_ensure_bytes(c, s.d_query, (size_t)qlen[0] + 64, false)) return GSA_ERR_NOMEM;
		size_t nb = (size_t)qlen[0];
#ifdef GSA_EXPERIMENTS
		{ static const long long cap = [] { const char *e = getenv("GSA_X_UPBYTES"); return e ? atoll(e) : -1ll; }(); if (cap >= 0 && (size_t)cap < nb) nb = (size_t)cap; }      // (timing experiment: the API pattern without the bytes)
#endif
		// (a buffer from gsa_host_alloc is pinned: one DMA transfer; pageable memory is staged by the runtime)
		if (nb > 0) { job.pieces.push_back({ s.d_query.p, query[0], nb }); c->up->push(std::move(job)); }
		return GSA_OK;
	}
	size_t t_bytes = 0;
	if (int rc = slot_tables(c, s, query, qlen, n, 4, &t_bytes)) return rc;
	uint8_t *ht = s.p_bndtab.as<uint8_t>();
	memcpy(ht + s.o_src, qlen, (size_t)n * 4);      // (the source column: the lengths, for k_bundle_pad)
	job.pieces.push_back({ s.d_bndtab.p, ht, t_bytes });
	for (int k = 0; k < n; k++) if (qlen[k] > 0) job.pieces.push_back({ s.d_query.as<uint8_t>() + s.b_off[(size_t)k], query[k], (size_t)qlen[k] });
	c->up->push(std::move(job));
	return GSA_OK;
}

// The host waits for the slot's upload (long over when the contig was prefetched a contig ago), then the main stream pads a bundle's contigs.
static int slot_finish(gsa_ctx *c, QuerySlot &s)
{
	slot_demand(c, s);
	if (const int e = s.up_err.exchange(0)) return gsa_fail(c, GSA_ERR_HIP, std::string("query upload (hipMemcpyAsync H2D): ") + hipGetErrorString((hipError_t)e));
	if (s.n > 0 && s.tot > 0) {
		const uint8_t *dt = s.d_bndtab.as<uint8_t>();
		hipLaunchKernelGGL(k_bundle_pad, dim3((unsigned)s.n), dim3(256), 0, c->stream, (const i32 *)dt, (const i32 *)(dt + s.o_src), s.d_query.as<uint8_t>());
		GSA_CHECK(c, hipGetLastError());
	}
	return GSA_OK;
}
static bool slot_holds(const QuerySlot &s, const char *const *query, const int32_t *qlen, int32_t n)
{
	if (!s.pending || s.n != n) return false;
	const int32_t m = n ? n : 1;
	if ((int32_t)s.src.size() != m || (int32_t)s.b_qlen.size() != m) return false;
	for (int32_t k = 0; k < m; k++) if (s.src[(size_t)k] != query[k] || s.b_qlen[(size_t)k] != qlen[k]) return false;
	return true;
}

// The slot the stages will read: the one a prefetch filled with exactly these buffers (the main stream waits for its upload), else a
// free one, filled on the main stream.
static int slot_acquire(gsa_ctx *c, const char *const *query, const int32_t *qlen, int32_t n, int *which)
{
	for (int i = 0; i < 2; i++) if (slot_holds(c->qs[i], query, qlen, n)) {
		c->qs[i].pending = false; *which = i;
		return slot_finish(c, c->qs[i]);
	}
	const int i = slot_pick_free(c);
	if (i < 0) return gsa_fail(c, GSA_ERR_STATE, "both query slots hold prefetched contigs: align them (or gsa_cancel_prefetch) first");
	*which = i;
	if (int rc = slot_upload(c, c->qs[i], query, qlen, n)) return rc;
	return slot_finish(c, c->qs[i]);
}
static int prefetch(gsa_ctx *c, const char *const *query, const int32_t *qlen, int32_t n)
{
	GSA_CHECK(c, hipSetDevice(c->device));
	// (the same buffer may wait twice -- a caller that aligns one buffer again and again -- so a waiting copy of it is no reason to skip this one)
	// not the slot of the contig that was aligned last while the other one is free (gsa_rewind stays possible); a pending slot never
	int i = c->q_cur == 0 ? 1 : 0;
	if (c->qs[i].pending) i ^= 1;
	if (c->qs[i].pending) return gsa_fail(c, GSA_ERR_STATE, "gsa_prefetch: two contigs are waiting already");
	// the only free slot holds the contig whose stages are under way (stage views: gsa_set_query + gsa_run_to(k < 8)): the later stages still
	// read its bases there -- overwriting, or growing and so freeing, that buffer would hand them another contig or freed memory
	if (i == c->q_cur && c->stage > 0 && c->stage < 8) return gsa_fail(c, GSA_ERR_STATE, "gsa_prefetch: the free query slot holds the contig whose stages are still running (finish it with gsa_run_to(8) or gsa_set_query first)");
	if (i == c->q_cur) c->q_cur = -2;
	int rc = slot_upload(c, c->qs[i], query, qlen, n);
	if (rc == GSA_OK) c->qs[i].pending = true;
	return rc;
}

// ---- several contigs in one pass (Bundle, gsa_internal.h): gsa_align_bundle's gsa_set_query ----
int set_query_bundle(gsa_ctx *c, const char *const *query, const int32_t *qlen, int32_t n, bool dev_q)
{
	if (n < 1 || n > GSA_BUNDLE_MAX_CONTIGS) return gsa_fail(c, GSA_ERR_ARG, "gsa_align_bundle: 1 .. 4096 contigs");
	GSA_CHECK(c, hipSetDevice(c->device));
	if (int rc = reset_run_state(c)) return rc;
	int w = 0;
	if (!dev_q) { if (int rc = slot_acquire(c, query, qlen, n, &w)) return rc; }
	else {
		// device-resident contigs: gathered into a free slot by one kernel (a workgroup per chunk), sources in the slot's table
		w = slot_pick_free(c);
		if (w < 0) return gsa_fail(c, GSA_ERR_STATE, "both query slots hold prefetched contigs");
		QuerySlot &s = c->qs[w];
		slot_wait(s);
		for (int k = 0; k < n; k++) if (qlen[k] > 0 && !device_ptr_of(c, query[k])) return gsa_fail(c, GSA_ERR_ARG, "gsa_align_bundle (GSA_MANY_DEVICE): not a device buffer of this context's GPU");
		size_t t_bytes = 0;
		if (int rc = slot_tables(c, s, query, qlen, n, sizeof(BundleSrc), &t_bytes)) return rc;
		BundleSrc *bs = (BundleSrc *)(s.p_bndtab.as<uint8_t>() + s.o_src);
		for (int k = 0; k < n; k++) { bs[k].p = (const uint8_t *)query[k]; bs[k].len = qlen[k]; bs[k]._pad = 0; }
		GSA_CHECK(c, hipMemcpyAsync(s.d_bndtab.p, s.p_bndtab.p, t_bytes, hipMemcpyHostToDevice, c->stream));
		const uint8_t *dt = s.d_bndtab.as<uint8_t>();
		if (s.tot > 0) {
			hipLaunchKernelGGL(k_bundle_gather, dim3((unsigned)(s.tot / GSA_CHUNK)), dim3(256), 0, c->stream, (const i32 *)dt, (const uint16_t *)(dt + s.o_cc), (const BundleSrc *)(dt + s.o_src), s.d_query.as<uint8_t>());
			GSA_CHECK(c, hipGetLastError());
		}
	}
	const QuerySlot &s = c->qs[w];
	const uint8_t *dt = s.d_bndtab.as<uint8_t>();
	c->q_cur = w; c->b_off = s.b_off; c->b_qlen = s.b_qlen; c->q_dev = s.d_query.as<uint8_t>();
	c->bnd.n = n; c->bnd.lmax = s.lmax; c->bnd.off = (const i32 *)dt; c->bnd.chunk_contig = (const uint16_t *)(dt + s.o_cc);
	c->bnd.pds = (2 * c->G + (i64)s.lmax + (i64)c->prm.MaxIndelSize + 64 + 31) & ~31ll;      // (a PosDiff of contig k: rPos - qLocal + lmax in (0, 2G + lmax])
	return seed_key_geometry(c, s.tot, (i64)n * c->bnd.pds + 2, "bundle");
}

extern "C" {
int gsa_prefetch_contig(gsa_ctx *c, const char *query, int32_t qlen)
{
	if (!c || !query || qlen < 0) return GSA_ERR_ARG;
	return prefetch(c, &query, &qlen, 0);
}
int gsa_prefetch_bundle(gsa_ctx *c, const char *const *query, const int32_t *qlen, int32_t n)
{
	if (!c || !query || !qlen) return GSA_ERR_ARG;
	if (n < 1 || n > GSA_BUNDLE_MAX_CONTIGS) return gsa_fail(c, GSA_ERR_ARG, "gsa_prefetch_bundle: 1 .. 4096 contigs");
	return prefetch(c, query, qlen, n);
}
int gsa_cancel_prefetch(gsa_ctx *c)
{
	if (!c) return GSA_ERR_ARG;
	c->qs[0].pending = c->qs[1].pending = false;      // (the copies run to their end; slot_upload waits for them before it reuses the slot)
	return GSA_OK;
}

int gsa_set_query(gsa_ctx *c, const char *query, int32_t qlen)
{
	if (!c || !query || qlen < 0) return GSA_ERR_ARG;
	GSA_CHECK(c, hipSetDevice(c->device));
	if (int rc = reset_run_state(c)) return rc;
	int w = 0;
	const auto t0 = std::chrono::steady_clock::now();
	if (int rc = slot_acquire(c, &query, &qlen, 0, &w)) return rc;
	c->wall_ms[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	c->q_cur = w; c->q_dev = c->qs[w].d_query.as<uint8_t>();
	return query_geometry(c, qlen);
}

// The contig is already in device memory (a loader that decodes FASTA on the GPU, or a contig kept resident between runs):
// used in place, no copy.
int gsa_set_query_device(gsa_ctx *c, const char *d_query, int32_t qlen)
{
	if (!c || !d_query || qlen < 0) return GSA_ERR_ARG;
	if (((uintptr_t)d_query & 15) != 0) return gsa_fail(c, GSA_ERR_ARG, "gsa_set_query_device: the buffer must be 16-byte aligned");
	GSA_CHECK(c, hipSetDevice(c->device));
	if (!device_ptr_of(c, d_query)) return gsa_fail(c, GSA_ERR_ARG, "gsa_set_query_device: not a device buffer of this context's GPU");
	if (int rc = reset_run_state(c)) return rc;
	c->q_dev = (const uint8_t *)d_query; c->q_cur = -1;
	return query_geometry(c, qlen);
}
} // extern "C"
