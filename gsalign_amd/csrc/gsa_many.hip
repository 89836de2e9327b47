// gsalign_amd/csrc/gsa_many.hip -- gsa_align_many*: many contigs on several contexts by the library's own worker threads.  Policy only: which context gets which
// contig, alone, split over a group of contexts or bundled with others; every contig itself goes through the align calls of gsa_api.hip.
#include <algorithm>
#include "gsa_ctx.h"

// One contig on a group of contexts (the first one owns it): IdentifyLocalMEM hands 10 000-bp chunks to whichever thread is free
// (GSAlign.cpp:61-94); here every context of the group seeds a contiguous chunk range, the owner imports the others' hits
// device to device and runs the rest.
static int align_split(gsa_ctx *const *grp, int n_grp, const char *query, int32_t qlen, gsa_result *out)
{
	const int32_t n_chunks = (int32_t)(((int64_t)qlen + GSA_CHUNK - 1) / GSA_CHUNK);
	std::vector<int> rcs((size_t)n_grp, GSA_OK);
	std::vector<std::thread> th;
	auto range = [&](int k, int32_t &b, int32_t &e) { const int32_t base = n_chunks / n_grp, extra = n_chunks % n_grp; b = k * base + (k < extra ? k : extra); e = b + base + (k < extra ? 1 : 0); };
	for (int k = 1; k < n_grp; k++) th.emplace_back([&, k] { int32_t b, e; range(k, b, e); rcs[(size_t)k] = gsa_seed_chunks(grp[k], query, qlen, b, e); });
	{ int32_t b, e; range(0, b, e); rcs[0] = gsa_seed_chunks(grp[0], query, qlen, b, e); }
	for (std::thread &t : th) t.join();
	for (int k = 0; k < n_grp; k++) if (rcs[(size_t)k] != GSA_OK) { if (k) gsa_fail(grp[0], rcs[(size_t)k], std::string("helper context: ") + gsa_last_error(grp[k])); return rcs[(size_t)k]; }
	for (int k = 1; k < n_grp; k++) {
		const uint64_t *kp = nullptr; const uint32_t *vp = nullptr;
		int rc = gsa_hit_buffers(grp[k], &kp, &vp);
		if (rc == GSA_OK) rc = gsa_import_hits(grp[0], kp, vp, gsa_hit_count(grp[k]));
		if (rc != GSA_OK) return rc;
	}
	return gsa_finish_contig(grp[0], out);
}

// Fewer contigs than contexts (BASELINE configs[3]: one chromosome, two GPUs): contexts would sit idle, so the contexts are
// dealt out in GROUPS, one per contig, sized by contig length, and every group seeds its contig by chunk range (align_split).
// Only contigs of at least GSA_SPLIT_MIN bases (default 20 Mb: below that the seed search is a fraction of a millisecond and
// a second upload of the contig costs more than it saves) get more than one context.  Returns the group size of every contig, in hand-out order.
static std::vector<int> deal_groups(const std::vector<int32_t> &order, const int32_t *qlen, int n_ctx, int64_t split_min)
{
	const int n = (int)order.size();
	std::vector<int> gsz((size_t)n, 1);
	for (int left = n_ctx - n; left > 0; left--) {       // the next context goes where a context has the most bases to itself
		int best = -1; double load = 0;
		for (int i = 0; i < n; i++) { const int32_t ci = order[(size_t)i]; if ((int64_t)qlen[ci] < split_min) continue; const double l = (double)qlen[ci] / gsz[(size_t)i]; if (l > load) { load = l; best = i; } }
		if (best < 0) break;
		gsz[(size_t)best]++;
	}
	return gsz;
}

// Short contigs travel in BUNDLES: a contig of a few Mb is ~60 GPU operations whatever its size, and with several contexts in
// flight the operations of one stretch the other's (profiles/archive/r03_timeline_multi_*.txt), so n short contigs are concatenated and
// go through the stages as ONE pass (set_query_bundle / gsa_align_bundle; results per contig, identical to the ones they get
// alone).  A unit of work = a long contig, or a bundle of consecutive short ones in hand-out order.  Bundle size: measured on
// 5 Mb contigs, larger is better all the way (6 / 11 / 16 / 21 / 31 / 60 Mb per bundle: 5.3 / 7.6 / 9.7 / 10.8 / 13.9 / 16.0 Gbp/s on
// one context, profiles/archive/r03_bundle_sweep.txt), so the short contigs are dealt into as few bundles as GSA_BUNDLE_CAP (default
// 64 Mb) allows, rounded up to a multiple of the context count (one equal share per context).  Contigs above
// GSA_BUNDLE_CONTIG (default 16 Mb) stay alone; GSA_BUNDLE_CONTIG=0 or GSA_MANY_NO_BUNDLE: no bundles; none either while a context
// is `profiling` (per-contig counters and stage timers).  Returns the units, contig numbers in hand-out order.
static std::vector<std::vector<int32_t> > plan_units(const std::vector<int32_t> &order, const int32_t *qlen, uint32_t flags, const Options &opt, i64 G, i32 MaxIndelSize, int n_ctx, bool profiling)
{
	const int64_t bundle_contig = opt.bundle_contig, bundle_cap = opt.bundle_cap;
	std::vector<std::vector<int32_t> > units;
	bool may = !(flags & GSA_MANY_NO_BUNDLE) && bundle_contig > 0 && !profiling;
	int64_t small_total = 0; int32_t n_small = 0;
	for (int32_t ci : order) if ((int64_t)qlen[ci] <= bundle_contig) { small_total += qlen[ci]; n_small++; }
	if (n_small < 2) may = false;
	// the 64-bit seed key holds (contig x stride + PosDiff, position in the bundle): against a large reference (stride ~ 2G) only
	// so many contigs fit one bundle -- 32 against a human genome
	size_t max_contigs = GSA_BUNDLE_MAX_CONTIGS;
	{
		const int qb = ceil_log2_u64((u64)(bundle_cap + bundle_cap / 8 + bundle_contig) + 1);
		const u64 stride = (u64)(2 * G) + (u64)bundle_contig + (u64)MaxIndelSize + 96;
		const u64 fit = qb < 62 ? (1ull << (63 - qb)) / stride : 0;
		if (fit < max_contigs) max_contigs = (size_t)fit;
		if (max_contigs < 2) may = false;
	}
#ifdef GSA_EXPERIMENTS
	static const int64_t bundle_target = [] { const char *e = getenv("GSA_BUNDLE_TARGET"); return e ? (int64_t)atoll(e) : 0ll; }();      // (a fixed bundle size)
#else
	const int64_t bundle_target = 0;
#endif
	int64_t n_bundles = (small_total + bundle_cap - 1) / (bundle_cap > 0 ? bundle_cap : 1); if (n_bundles < 1) n_bundles = 1;
	n_bundles = (n_bundles + n_ctx - 1) / n_ctx * n_ctx;
	int64_t target = small_total / n_bundles + 1;
	if (bundle_target > 0) target = bundle_target;
	int64_t cur = 0;
	for (int32_t ci : order) {
		const bool small = may && (int64_t)qlen[ci] <= bundle_contig;
		if (!small) { units.push_back(std::vector<int32_t>(1, ci)); cur = 0; continue; }
		const int64_t padded = ((int64_t)qlen[ci] + GSA_CHUNK - 1) / GSA_CHUNK * GSA_CHUNK;
		if (cur > 0 && (cur + padded / 2 > target || cur + padded > bundle_cap + bundle_cap / 8 || units.back().size() >= max_contigs)) cur = 0;      // (to the nearest contig)
		if (cur == 0) units.push_back(std::vector<int32_t>());
		units.back().push_back(ci); cur += padded > 0 ? padded : 1;
	}
	return units;
}

// what the callback of gsa_align_many_ex is handed: the public gsa_extras at the head, the answers of later passes behind it
struct ExtrasFull { gsa_extras ex; const gsa_cs *cs; const gsa_lifts *lift; const gsa_tracks *track; const gsa_segs *segs; const gsa_region_lifts *regions; const gsa_qtracks *qtrack; };
// gsa_align_many, gsa_align_many_variants and gsa_align_many_ex: one loop, three ways to hand a finished contig over (the passes asked for run first, in the worker that finished it)
struct ManySink { gsa_result_fn on_result = nullptr; gsa_result_var_fn on_var = nullptr; gsa_result_ex_fn on_ex = nullptr; uint32_t want = 0; };
static int align_many_impl(gsa_ctx *const *ctx, int32_t n_ctx, const char *const *query, const int32_t *qlen, int32_t n, uint32_t flags, const ManySink &sk, void *user)
{
	// contig `ci` is finished on context c (contig k of the bundle c holds, 0 otherwise): the current contig's device copy is still in its slot here -- the
	// prefetch of the unit after next is only issued once this unit's callbacks have returned
	auto deliver = [&](gsa_ctx *c, int32_t k, int32_t ci, const gsa_result *res) -> int {
		if (sk.on_var) { gsa_variants var; const int rcv = gsa_call_variants(c, k, &var); return rcv != GSA_OK ? rcv : sk.on_var(user, ci, res, &var); }
		if (sk.on_ex) {
			gsa_variants var; gsa_cigars cig; gsa_cs cs; gsa_lifts lift; gsa_tracks trk; gsa_segs sg; gsa_region_lifts rg; gsa_qtracks qtk; ExtrasFull full = { { nullptr, nullptr }, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr }; gsa_extras &ex = full.ex;
			// (the variants are copied by no one before the CIGAR pass runs, and both live in buffers of their own: the second pass leaves the first one's answer alone)
			if (sk.want & GSA_WANT_VARIANTS) { const int rcv = gsa_call_variants(c, k, &var); if (rcv != GSA_OK) return rcv; ex.var = &var; }
			// (the cs pass runs the CIGAR walk itself, into the CIGAR pass's buffers: its ops are the ones handed out, no second walk)
			if (sk.want & GSA_WANT_CS) { const int rcs = cs_call(c, k, &cs, &cig); if (rcs != GSA_OK) return rcs; full.cs = &cs; ex.cig = &cig; }
			// (the segs pass runs the CIGAR walk itself too -- behind the cs pass it reads what that walk has just left on the device, no second walk; its ops are the ones handed out)
			if (sk.want & GSA_WANT_SEGS) { const bool walked = (sk.want & GSA_WANT_CS) != 0; const int rcg = segs_call(c, k, &sg, walked ? nullptr : &cig, walked ? &cig : nullptr); if (rcg != GSA_OK) return rcg; full.segs = &sg; ex.cig = &cig; }
			else if (!(sk.want & GSA_WANT_CS) && (sk.want & GSA_WANT_CIGARS)) { const int rcc = gsa_block_cigars(c, k, &cig); if (rcc != GSA_OK) return rcc; ex.cig = &cig; }
			if (sk.want & GSA_WANT_LIFT) { const int rcl = lift_call(c, k, &lift); if (rcl != GSA_OK) return rcl; full.lift = &lift; }
			if (sk.want & GSA_WANT_TRACK) { const int rct = track_call(c, k, &trk); if (rct != GSA_OK) return rct; full.track = &trk; }
			if (sk.want & GSA_WANT_REGIONS) { const int rcr = regions_call(c, k, &rg); if (rcr != GSA_OK) return rcr; full.regions = &rg; }
			if (sk.want & GSA_WANT_QTRACK) { const int rcq = qtrack_call(c, k, &qtk); if (rcq != GSA_OK) return rcq; full.qtrack = &qtk; }
			// (the projection paints into the contexts' accumulator and hands the callback nothing)
			if (sk.want & GSA_WANT_PROJ) { const int rcp = proj_call(c, k, nullptr); if (rcp != GSA_OK) return rcp; }
			return sk.on_ex(user, ci, res, &ex);
		}
		return sk.on_result ? sk.on_result(user, ci, res) : GSA_OK;
	};
	if (flags & ~(uint32_t)(GSA_MANY_IN_ORDER | GSA_MANY_DEVICE | GSA_MANY_NO_SPLIT | GSA_MANY_NO_BUNDLE | GSA_MANY_NO_PREFETCH)) return GSA_ERR_ARG;
	if (!ctx || n_ctx <= 0 || n < 0 || (n > 0 && (!query || !qlen))) return GSA_ERR_ARG;
	for (int k = 0; k < n_ctx; k++) if (!ctx[k]) return GSA_ERR_ARG;
	const bool dev_q = (flags & GSA_MANY_DEVICE) != 0;
	if (dev_q) for (int k = 1; k < n_ctx; k++) if (ctx[k]->device != ctx[0]->device) return gsa_fail(ctx[0], GSA_ERR_ARG, "GSA_MANY_DEVICE: the contexts must share one GPU (the contigs live in its memory)");
	// (what a pass reads must be set on every context: one without would fail its first contig with the others under way)
	static const struct { uint32_t want; bool (*set)(const gsa_ctx *); const char *msg; } needs[4] = {
		{ GSA_WANT_LIFT, [](const gsa_ctx *c) { return c->lift_n > 0; }, "gsa_align_many_ex (GSA_WANT_LIFT): the context holds no positions (gsa_lift_set first)" },
		{ GSA_WANT_TRACK, [](const gsa_ctx *c) { return c->track_w > 0; }, "gsa_align_many_ex (GSA_WANT_TRACK): the context holds no window (gsa_track_set first)" },
		{ GSA_WANT_QTRACK, [](const gsa_ctx *c) { return c->qtrack_w > 0; }, "gsa_align_many_ex (GSA_WANT_QTRACK): the context holds no query-side window (gsa_qtrack_set first)" },
		{ GSA_WANT_REGIONS, [](const gsa_ctx *c) { return c->reg_n > 0; }, "gsa_align_many_ex (GSA_WANT_REGIONS): the context holds no regions (gsa_regions_set first)" } };
	for (const auto &nd : needs) if (sk.want & nd.want) for (int k = 0; k < n_ctx; k++) if (!nd.set(ctx[k])) return gsa_fail(ctx[k], GSA_ERR_STATE, nd.msg);
	// (GSA_WANT_PROJ: the bit exists for callers that have opened an accumulator.  Where NO context of ctx[] holds one it is refused like any bit the call does not know --
	//  GSA_ERR_ARG, what 128 gave before the pass existed; where some hold one and others do not, the call is half set up: GSA_ERR_STATE.  Either way before any contig is aligned)
	if (sk.want & GSA_WANT_PROJ) {
		int held = 0;
		for (int k = 0; k < n_ctx; k++) if (ctx[k]->proj) held++;
		if (held == 0) return gsa_fail(ctx[0], GSA_ERR_ARG, "gsa_align_many_ex (GSA_WANT_PROJ): no context holds an accumulator (gsa_proj_open first)");
		for (int k = 0; k < n_ctx; k++) if (!ctx[k]->proj) return gsa_fail(ctx[k], GSA_ERR_STATE, "gsa_align_many_ex (GSA_WANT_PROJ): the context holds no accumulator (gsa_proj_open first)");
	}
	if (n == 0) return GSA_OK;
	// longest first: with dynamic hand-out this is the longest-processing-time-first rule
	std::vector<int32_t> order((size_t)n);
	for (int32_t i = 0; i < n; i++) order[(size_t)i] = i;
	if (!(flags & GSA_MANY_IN_ORDER)) std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return qlen[a] > qlen[b]; });
	std::atomic<int> err(GSA_OK);
	const int64_t split_min = ctx[0]->opt.split_min;
	int64_t longest = 0; for (int32_t i = 0; i < n; i++) if (qlen[i] > longest) longest = qlen[i];      // (in hand-out order the first contig need not be the longest)
	if (n < n_ctx && !dev_q && !(flags & GSA_MANY_NO_SPLIT) && longest >= split_min) {
		const std::vector<int> gsz = deal_groups(order, qlen, n_ctx, split_min);
		std::vector<std::thread> th; int at = 0;
		for (int i = 0; i < n; i++) {
			const int32_t ci = order[(size_t)i]; gsa_ctx *const *grp = ctx + at; const int ng = gsz[(size_t)i]; at += ng;
			th.emplace_back([&, ci, grp, ng] {
				gsa_result res;
				int rc = ng > 1 ? align_split(grp, ng, query[ci], qlen[ci], &res) : gsa_align_contig(grp[0], query[ci], qlen[ci], &res);
				if (rc == GSA_OK) rc = deliver(grp[0], 0, ci, &res);
				if (rc != GSA_OK) { int ok = GSA_OK; err.compare_exchange_strong(ok, rc); }
			});
		}
		for (std::thread &t : th) t.join();
		return err.load();
	}
	bool profiling = false;
	for (int k = 0; k < n_ctx; k++) if (ctx[k]->profiling || ctx[k]->count_blocks) profiling = true;
	const std::vector<std::vector<int32_t> > units = plan_units(order, qlen, flags, ctx[0]->opt, ctx[0]->G, ctx[0]->prm.MaxIndelSize, n_ctx, profiling);
	const int32_t n_units = (int32_t)units.size();
	std::atomic<int32_t> next(0);
	auto one = [&](gsa_ctx *c, int32_t ci) {
		gsa_result res;
		int rc = dev_q ? gsa_align_contig_device(c, query[ci], qlen[ci], &res) : gsa_align_contig(c, query[ci], qlen[ci], &res);
		if (rc == GSA_OK) rc = deliver(c, 0, ci, &res);
		return rc;
	};
	// A context works on unit u while unit u + 1 -- claimed one ahead -- is uploaded into its other query slot (gsa_prefetch_contig /
	// gsa_prefetch_bundle): the reference reads a sequence from host memory when its turn comes (GSAlign.cpp:483-490); here the H2D
	// copy of a chromosome (4.8 ms per 250 Mb) would otherwise sit in front of every contig's seed search.
	const bool pre = !dev_q && !(flags & GSA_MANY_NO_PREFETCH);
	auto loop = [&](gsa_ctx *c) {
		std::vector<const char *> bq, pq; std::vector<int32_t> bl, pl; std::vector<gsa_result> br;
		auto fetch = [&](int32_t u) {
			if (!pre || u >= n_units) return;
			const std::vector<int32_t> &un = units[(size_t)u];
			if (un.size() == 1) (void)gsa_prefetch_contig(c, query[un[0]], qlen[un[0]]);
			else { pq.clear(); pl.clear(); for (int32_t ci : un) { pq.push_back(query[ci]); pl.push_back(qlen[ci]); } (void)gsa_prefetch_bundle(c, pq.data(), pl.data(), (int32_t)un.size()); }
			// (a prefetch that fails -- memory -- leaves nothing pending: the contig is uploaded when its turn comes)
		};
		(void)gsa_cancel_prefetch(c);
		int32_t u = next.fetch_add(1);
		fetch(u);
		for (;;) {
			if (u >= n_units || err.load() != GSA_OK) { (void)gsa_cancel_prefetch(c); return; }
			const int32_t u_next = next.fetch_add(1);
			fetch(u_next);
			const std::vector<int32_t> &un = units[(size_t)u];
			int rc = GSA_OK;
			if (un.size() == 1) rc = one(c, un[0]);
			else {
				bq.clear(); bl.clear(); br.resize(un.size());
				for (int32_t ci : un) { bq.push_back(query[ci]); bl.push_back(qlen[ci]); }
				rc = gsa_align_bundle(c, bq.data(), bl.data(), (int32_t)un.size(), dev_q ? GSA_MANY_DEVICE : 0u, br.data());
				if (rc == GSA_OK) { for (size_t k = 0; k < un.size() && rc == GSA_OK; k++) rc = deliver(c, (int32_t)k, un[k], &br[k]); }
				else if (rc == GSA_ERR_LIMIT) { rc = GSA_OK; for (size_t k = 0; k < un.size() && rc == GSA_OK; k++) rc = one(c, un[k]); }      // (a capacity of the joint pass: one by one)
			}
			if (rc != GSA_OK) { int ok = GSA_OK; err.compare_exchange_strong(ok, rc); (void)gsa_cancel_prefetch(c); return; }
			u = u_next;
		}
	};
	std::vector<std::thread> th;
	// (thread placement is the caller's: gsa_bind_host_thread; the threads started here inherit the caller's affinity)
	for (int k = 1; k < n_ctx && k < n_units; k++) th.emplace_back(loop, ctx[k]);
	loop(ctx[0]);
	for (std::thread &t : th) t.join();
	return err.load();
}

// one answer of a later pass behind the public gsa_extras: zeroed, then the pass's if it ran (GSA_ERR_STATE: it was not asked for)
template <class T>
static int extras_get(const gsa_extras *ex, const T *ExtrasFull::*which, T *out)
{
	if (!ex || !out) return GSA_ERR_ARG;
	*out = T();
	const T *p = ((const ExtrasFull *)ex)->*which;
	if (!p) return GSA_ERR_STATE;
	*out = *p;
	return GSA_OK;
}

extern "C" {
int gsa_align_many(gsa_ctx *const *ctx, int32_t n_ctx, const char *const *query, const int32_t *qlen, int32_t n, uint32_t flags, gsa_result_fn on_result, void *user)
{
	ManySink sk; sk.on_result = on_result;
	return align_many_impl(ctx, n_ctx, query, qlen, n, flags, sk, user);
}
int gsa_align_many_variants(gsa_ctx *const *ctx, int32_t n_ctx, const char *const *query, const int32_t *qlen, int32_t n, uint32_t flags, gsa_result_var_fn on_result, void *user)
{
	if (!on_result) return GSA_ERR_ARG;
	ManySink sk; sk.on_var = on_result;
	return align_many_impl(ctx, n_ctx, query, qlen, n, flags, sk, user);
}
int gsa_align_many_ex(gsa_ctx *const *ctx, int32_t n_ctx, const char *const *query, const int32_t *qlen, int32_t n, uint32_t flags, uint32_t want, gsa_result_ex_fn on_result, void *user)
{
	if (!on_result || (want & ~(uint32_t)(GSA_WANT_VARIANTS | GSA_WANT_CIGARS | GSA_WANT_CS | GSA_WANT_LIFT | GSA_WANT_TRACK | GSA_WANT_SEGS | GSA_WANT_PROJ | GSA_WANT_REGIONS | GSA_WANT_QTRACK))) return GSA_ERR_ARG;
	ManySink sk; sk.on_ex = on_result; sk.want = want;
	return align_many_impl(ctx, n_ctx, query, qlen, n, flags, sk, user);
}

// the answers behind the gsa_extras a gsa_align_many_ex callback was handed: cs strings (GSA_WANT_CS), lifted positions (GSA_WANT_LIFT), chain segments (GSA_WANT_SEGS),
// the per-window track (GSA_WANT_TRACK), lifted regions (GSA_WANT_REGIONS), the per-window query track (GSA_WANT_QTRACK)
int gsa_extras_cs(const gsa_extras *ex, gsa_cs *out) { return extras_get(ex, &ExtrasFull::cs, out); }
int gsa_extras_lift(const gsa_extras *ex, gsa_lifts *out) { return extras_get(ex, &ExtrasFull::lift, out); }
int gsa_extras_segs(const gsa_extras *ex, gsa_segs *out) { return extras_get(ex, &ExtrasFull::segs, out); }
int gsa_extras_track(const gsa_extras *ex, gsa_tracks *out) { return extras_get(ex, &ExtrasFull::track, out); }
int gsa_extras_regions(const gsa_extras *ex, gsa_region_lifts *out) { return extras_get(ex, &ExtrasFull::regions, out); }
int gsa_extras_qtrack(const gsa_extras *ex, gsa_qtracks *out) { return extras_get(ex, &ExtrasFull::qtrack, out); }
} // extern "C"
