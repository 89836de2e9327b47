// gsalign_amd/csrc/host/host_api.cpp -- C entry points of libgsa_host.so, so that
// the CPU test-suite can drive the host-side components (index builder, loader,
// emitters) without a GPU.  The CLI uses the C++ interface directly.
#include <atomic>
#include <algorithm>
#include <cstring>
#include <mutex>
#include "gsa_host.h"
#include "par.h"
#include "exact_sort.h"

extern "C" {

// LoadQueryFile through the C API (tests): the contigs stay in a static list until the next call
static std::vector<QueryContig> g_query;
int gsah_c_load_query(const char *path, char *err)
{
	g_query.clear(); std::string e;
	if (gsah_load_query(path, g_query, e)) return (int)g_query.size();
	if (err) { strncpy(err, e.c_str(), 255); err[255] = 0; }
	g_query.clear();
	return -1;
}
const char *gsah_c_query_name(int i) { return g_query[(size_t)i].name.c_str(); }
long long gsah_c_query_len(int i) { return (long long)g_query[(size_t)i].seq.size(); }
const char *gsah_c_query_seq(int i) { return g_query[(size_t)i].seq.data(); }

// exact_sort (exact_sort.h) against std::sort itself on n keys {a, b, original index} compared on (a, b) only -- the VCF sort's shape.
// pattern 0: random with `distinct` values per field (ties), 1: ascending, 2: descending, 3: all equal, 4: organ pipe, 5: a few long runs, 6: the
// median-of-three killer (quicksort's depth budget runs out: the heapsort fallback).  Returns 0 when every element sits where std::sort put it.
int gsah_c_exact_sort_check(long long n, int distinct, unsigned seed, int pattern, long long grain)
{
	struct Key { int32_t a, b; uint32_t idx, pad; };
	struct ByAB { bool operator()(const Key &x, const Key &y) const { return x.a == y.a ? x.b < y.b : x.a < y.a; } };
	std::vector<Key> v((size_t)n);
	unsigned long long st = seed * 2654435761ull + 88172645463325252ull;
	auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
	for (long long i = 0; i < n; i++) {
		Key k; k.idx = (uint32_t)i; k.pad = 0;
		switch (pattern) {
		case 1: k.a = 0; k.b = (int32_t)(i / 3); break;
		case 2: k.a = 0; k.b = (int32_t)((n - i) / 3); break;
		case 3: k.a = 7; k.b = 7; break;
		case 4: k.a = 0; k.b = (int32_t)(i < n / 2 ? i : n - i); break;
		case 5: k.a = (int32_t)(i * 5 / (n > 0 ? n : 1)); k.b = (int32_t)(rnd() % 3); break;
		default: k.a = (int32_t)(rnd() % (unsigned)(distinct < 1 ? 1 : distinct)) / 97; k.b = (int32_t)(rnd() % (unsigned)(distinct < 1 ? 1 : distinct)); break;
		}
		v[(size_t)i] = k;
	}
	if (pattern == 6 && n >= 4) {      // Musser's median-of-three killer on b
		const long long k2 = n / 2;
		for (long long i = 0; i < k2; i++) { v[(size_t)i].a = 0; v[(size_t)i].b = (i % 2 == 0) ? (int32_t)(i + 1) : (int32_t)(k2 + i + (k2 % 2 ? 0 : 1)); }
		for (long long i = k2; i < n; i++) { v[(size_t)i].a = 0; v[(size_t)i].b = (int32_t)((i - k2 + 1) * 2); }
	}
	std::vector<Key> w(v);
	std::sort(v.begin(), v.end(), ByAB());
	exact_sort(w.data(), w.data() + w.size(), ByAB(), grain > 0 ? (size_t)grain : (size_t)1 << 16);
	for (size_t i = 0; i < v.size(); i++) if (v[i].idx != w[i].idx) return 1;
	return 0;
}

// returns 0 on success; err (>= 256 bytes) receives the message otherwise
// HostPool::run back to back with short jobs of changing size (the shape maf_block produces): every index of every run exactly once.
// Returns 0, or the 1-based run in which an index ran twice or not at all.  (Round-5 advisor finding: a worker that woke late could carry an
// index of the previous job into the next one.)
int gsah_c_pool_stress(int threads, int runs, unsigned seed)
{
	HostPool pool(threads);
	std::vector<std::atomic<int>> hit(4096);
	unsigned x = seed * 2654435761u + 1u;
	for (int r = 0; r < runs; r++) {
		x = x * 1664525u + 1013904223u;
		const size_t n = 2 + (x >> 20) % 4094;
		for (size_t i = 0; i < n; i++) hit[i].store(0, std::memory_order_relaxed);
		pool.run(n, [&](size_t i) { hit[i].fetch_add(1, std::memory_order_relaxed); });
		for (size_t i = 0; i < n; i++) if (hit[i].load(std::memory_order_relaxed) != 1) return r + 1;
	}
	return 0;
}

int gsah_c_build_index(const char *fasta, const char *prefix, char *err)
{
	std::string e;
	if (gsah_build_index(fasta, prefix, e)) return 0;
	if (err) { strncpy(err, e.c_str(), 255); err[255] = 0; }
	return -1;
}

// the builder with the BWT/SA half from a callback (gsah_bwt_fn; NULL: the host path)
int gsah_c_build_index_with(const char *fasta, const char *prefix, gsah_bwt_fn fn, void *user, char *err)
{
	std::string e;
	if (gsah_build_index_with(fasta, prefix, e, fn, user)) return 0;
	if (err) { strncpy(err, e.c_str(), 255); err[255] = 0; }
	return -1;
}

// gsah_reference_from_fasta through the C API: the reference stays in a static HostIndex until the next call; returns the number of sequences, -1 on error
static HostIndex g_ref;
int gsah_c_reference_from_fasta(const char *fasta, long long *G, long long *pac_bytes, char *err)
{
	std::string e;
	if (!gsah_reference_from_fasta(fasta, g_ref, e)) { if (err) { strncpy(err, e.c_str(), 255); err[255] = 0; } return -1; }
	*G = (long long)g_ref.G; *pac_bytes = (long long)g_ref.pac.size();
	return (int)g_ref.chr_len.size();
}
const unsigned char *gsah_c_reference_pac(void) { return g_ref.pac.data(); }
const char *gsah_c_reference_name(int i) { return g_ref.chr_name[(size_t)i].c_str(); }
int gsah_c_reference_len(int i) { return g_ref.chr_len[(size_t)i]; }

// Emit MAF + VCF for a whole query FASTA given, per contig, a finished gsa_result.
// get_result(user, contig_index, seq, len, &result) is called once per contig, in order.
typedef int (*gsah_result_cb)(void *user, int contig, const char *seq, int len, gsa_result *out);

int gsah_c_emit_fmt(const char *index_prefix, const char *query_fa, const char *maf_path, const char *vcf_path, const char *reference_label,
                    int allow_dup, int fmt, gsah_result_cb cb, void *user, char *err);

int gsah_c_emit(const char *index_prefix, const char *query_fa, const char *maf_path, const char *vcf_path, const char *reference_label,
                int allow_dup, gsah_result_cb cb, void *user, char *err)
{
	return gsah_c_emit_fmt(index_prefix, query_fa, maf_path, vcf_path, reference_label, allow_dup, 1, cb, user, err);
}

static int emit_impl(const char *index_prefix, const char *query_fa, const char *maf_path, const char *vcf_path, const char *reference_label,
                     int allow_dup, int fmt, bool with_cs, gsah_result_cb cb, void *user, char *err, const char *chain_path = nullptr);

// fmt 1: MAF (OutputMAF), fmt 2: ALN (OutputAlignment) -- the -fmt flag of the CLI (main.cpp:284); fmt 3: PAF, the CIGARs from the host comparator (gsah_block_cigars)
int gsah_c_emit_fmt(const char *index_prefix, const char *query_fa, const char *maf_path, const char *vcf_path, const char *reference_label,
                    int allow_dup, int fmt, gsah_result_cb cb, void *user, char *err)
{
	return emit_impl(index_prefix, query_fa, maf_path, vcf_path, reference_label, allow_dup, fmt, false, cb, user, err);
}

// fmt 3 with a cs:Z: field behind every cg:Z: (the -cs flag of the CLI): CIGARs and cs strings from the host comparators (gsah_block_cigars, gsah_block_cs)
int gsah_c_emit_paf_cs(const char *index_prefix, const char *query_fa, const char *paf_path, const char *vcf_path, const char *reference_label,
                       int allow_dup, gsah_result_cb cb, void *user, char *err)
{
	return emit_impl(index_prefix, query_fa, paf_path, vcf_path, reference_label, allow_dup, 3, true, cb, user, err);
}

// any of those with a UCSC chain file beside it (the -chain flag of the CLI): triples from the host comparator (gsah_block_segs), cut and printed by Emitter::chain
int gsah_c_emit_chain(const char *index_prefix, const char *query_fa, const char *maf_path, const char *vcf_path, const char *reference_label,
                      int allow_dup, int fmt, int with_cs, const char *chain_path, gsah_result_cb cb, void *user, char *err)
{
	if (!chain_path) return -1;
	return emit_impl(index_prefix, query_fa, maf_path, vcf_path, reference_label, allow_dup, fmt, with_cs != 0 && fmt == 3, cb, user, err, chain_path);
}

static int emit_impl(const char *index_prefix, const char *query_fa, const char *maf_path, const char *vcf_path, const char *reference_label,
                     int allow_dup, int fmt, bool with_cs, gsah_result_cb cb, void *user, char *err, const char *chain_path)
{
	std::string e; HostIndex idx; std::vector<QueryContig> qs;
	if (!gsah_load_index(index_prefix, idx, e) || !gsah_load_query(query_fa, qs, e)) { if (err) { strncpy(err, e.c_str(), 255); err[255] = 0; } return -1; }
	Emitter em; em.idx = &idx; em.allow_dup = allow_dup != 0;
	FILE *chain_fp = nullptr; int64_t chain_id = 0;
	if (chain_path && !(chain_fp = fopen(chain_path, "w"))) { if (err) strcpy(err, "cannot open chain output"); return -3; }
	struct Closer { FILE *&f; ~Closer() { if (f) fclose(f); } } closer = { chain_fp };
	for (size_t ci = 0; ci < qs.size(); ci++) {
		gsa_result res; memset(&res, 0, sizeof(res));
		if (cb(user, (int)ci, qs[ci].seq.data(), (int)qs[ci].seq.size(), &res) != 0) { if (err) strcpy(err, "result callback failed"); return -2; }
		if (res.n_blocks == 0) continue;                         // GSAlign.cpp:541
		ContigResult cr; cr.assign(res);
		if (chain_fp) em.chain(chain_fp, qs[ci], cr, nullptr, nullptr, &chain_id);      // (in front of the emitters that shorten a block's last record)
		FILE *fp = fopen(maf_path, ci == 0 ? "w" : "a");         // tools.cpp:158-163
		if (!fp) { if (err) strcpy(err, "cannot open MAF output"); return -3; }
		if (fmt == 3 && with_cs) {
			std::vector<gsa_block_cigar> cb_blk; std::vector<uint32_t> cb_ops; std::vector<gsa_cs_block> cs_blk; std::string cs;
			gsah_block_cigars(qs[ci].seq.data(), cr, cb_blk, cb_ops); gsah_block_cs(cr, cs_blk, cs);
			em.paf(fp, qs[ci], cr, cb_blk.data(), cb_ops.data(), cs_blk.data(), cs.data());
		} else if (fmt == 3) em.paf(fp, qs[ci], cr, nullptr, nullptr); else if (fmt == 2) em.aln(fp, qs[ci], cr); else em.maf(fp, ci == 0, qs[ci], cr);
		fclose(fp);
		em.variants((int)ci, qs[ci], cr);
	}
	FILE *fp = fopen(vcf_path, "w");
	if (!fp) { if (err) strcpy(err, "cannot open VCF output"); return -3; }
	em.vcf(fp, reference_label); fclose(fp);
	return 0;
}

// PAF from SUMMARY results (ContigResult::summary): per contig the callback supplies the FULL result; its CIGARs come from the host comparator and its
// block ends (first and last record of every block, as they lie in the full result) are taken out of it, and the PAF is then formatted from a ContigResult that holds only
// the blocks and those ends.  No VCF: the host variant walk needs the strings.
int gsah_c_emit_summary(const char *index_prefix, const char *query_fa, const char *paf_path, int allow_dup, gsah_result_cb cb, void *user, char *err)
{
	std::string e; HostIndex idx; std::vector<QueryContig> qs;
	if (!gsah_load_index(index_prefix, idx, e) || !gsah_load_query(query_fa, qs, e)) { if (err) { strncpy(err, e.c_str(), 255); err[255] = 0; } return -1; }
	Emitter em; em.idx = &idx; em.allow_dup = allow_dup != 0;
	for (size_t ci = 0; ci < qs.size(); ci++) {
		gsa_result res; memset(&res, 0, sizeof(res));
		if (cb(user, (int)ci, qs[ci].seq.data(), (int)qs[ci].seq.size(), &res) != 0) { if (err) strcpy(err, "result callback failed"); return -2; }
		if (res.n_blocks == 0) continue;
		std::vector<gsa_block_cigar> cb_blk; std::vector<uint32_t> cb_ops;
		std::vector<gsa_rec> ends((size_t)2 * (size_t)res.n_blocks);
		{
			ContigResult full; full.assign(res);
			gsah_block_cigars(qs[ci].seq.data(), full, cb_blk, cb_ops);
			for (int32_t b = 0; b < res.n_blocks; b++) {
				const gsa_block &bl = res.blocks[b];
				if (bl.n_frag <= 0) { memset(&ends[2 * (size_t)b], 0, 2 * sizeof(gsa_rec)); continue; }
				ends[2 * (size_t)b] = res.recs[bl.frag_off]; ends[2 * (size_t)b + 1] = res.recs[bl.frag_off + bl.n_frag - 1];
			}
		}
		gsa_result sum; memset(&sum, 0, sizeof(sum));
		sum.n_blocks = res.n_blocks; sum.blocks = res.blocks; sum.n_frags = (int64_t)ends.size(); sum.recs = ends.data();      // n_aln = 0, aln1 = aln2 = NULL
		ContigResult cr; cr.assign(sum, true);
		FILE *fp = fopen(paf_path, ci == 0 ? "w" : "a");
		if (!fp) { if (err) strcpy(err, "cannot open PAF output"); return -3; }
		em.paf(fp, qs[ci], cr, cb_blk.data(), cb_ops.data());
		fclose(fp);
	}
	return 0;
}

// VariantIdentification (SeqVariant.cpp:12-119) of one finished contig as gsa_variant records, on the host: the records gsa_call_variants gives, in the same
// order.  out[cap]; returns the number of variants (call with cap = 0 to size `out`), < 0 on error.  counts = {SNVs, insertions, deletions}.  `seq` is not read: the
// records address the alleles (gsa_variant_alleles).  The index of the last prefix stays loaded, behind a lock: calls from several threads take turns.
long long gsah_c_variants(const char *index_prefix, const char *seq, int len, const gsa_result *res, gsa_variant *out, long long cap, long long counts[3])
{
	static std::mutex mu; static std::string have; static HostIndex *idx = nullptr;
	std::lock_guard<std::mutex> lock(mu);
	(void)seq; (void)len;
	if (!index_prefix || !res || !counts || (cap > 0 && !out)) return -1;
	if (!idx || have != index_prefix) {
		delete idx; idx = new HostIndex; have.clear(); std::string e;
		if (!gsah_load_index(index_prefix, *idx, e)) { delete idx; idx = nullptr; return -2; }
		have = index_prefix;
	}
	ContigResult cr; cr.assign(*res);
	int64_t cnt[3];
	const int64_t n = gsah_variant_records(idx, cr, out, cap, cnt);
	for (int k = 0; k < 3; k++) counts[k] = cnt[k];
	return n;
}

// The CIGAR of every block of one finished contig (gsa_block_cigar / ops, gsa_hip.h), on the host, from the gapped strings and seed records, untrimmed: what
// gsa_block_cigars gives.  blk[res->n_blocks] is always filled; ops[cap]; returns the number of ops (call with cap = 0 to size `ops`), < 0 on error.
// seq (may be NULL): the query contig -- seed columns are then classified from its text.  Needs no index.
long long gsah_c_cigars(const char *seq, int len, const gsa_result *res, gsa_block_cigar *blk, uint32_t *ops, long long cap)
{
	(void)len;
	if (!res || (res->n_blocks > 0 && !blk) || (cap > 0 && !ops)) return -1;
	ContigResult cr; cr.assign(*res);
	std::vector<gsa_block_cigar> b; std::vector<uint32_t> o;
	gsah_block_cigars(seq, cr, b, o);
	if (!b.empty()) memcpy(blk, b.data(), b.size() * sizeof(gsa_block_cigar));
	const size_t m = std::min<size_t>(o.size(), cap > 0 ? (size_t)cap : 0);
	if (m) memcpy(ops, o.data(), m * sizeof(uint32_t));
	return (long long)o.size();
}

// gsah_cigar_trim on one block's ops (n = bc->n_cig of them): out[n] receives the ops that stay, *bc the reduced counts; returns their number
int gsah_c_cigar_trim(const uint32_t *ops, int bdir, long long ext, uint32_t *out, gsa_block_cigar *bc)
{
	if (!bc || (bc->n_cig > 0 && (!ops || !out))) return -1;
	std::vector<uint32_t> o;
	gsah_cigar_trim(ops, bdir, ext, o, *bc);
	if (!o.empty()) memcpy(out, o.data(), o.size() * sizeof(uint32_t));
	return (int)o.size();
}

// The cs string of every block of one finished contig (gsa_cs_block / bytes, gsa_hip.h), on the host, from the gapped strings and seed records, untrimmed: what
// gsa_block_cs gives.  blk[res->n_blocks] is always filled; cs[cap]; returns the number of bytes (call with cap = 0 to size `cs`), < 0 on error.  Needs no index.
long long gsah_c_cs(const gsa_result *res, gsa_cs_block *blk, char *cs, long long cap)
{
	if (!res || (res->n_blocks > 0 && !blk) || (cap > 0 && !cs)) return -1;
	ContigResult cr; cr.assign(*res);
	std::vector<gsa_cs_block> b; std::string o;
	gsah_block_cs(cr, b, o);
	if (!b.empty()) memcpy(blk, b.data(), b.size() * sizeof(gsa_cs_block));
	const size_t m = std::min<size_t>(o.size(), cap > 0 ? (size_t)cap : 0);
	if (m) memcpy(cs, o.data(), m);
	return (long long)o.size();
}

// gsah_cs_trim on one block's string cs[n] (of its untrimmed ops[n_ops]): out[n] receives the string that stays; returns its length
long long gsah_c_cs_trim(const char *cs, long long n, const uint32_t *ops, long long n_ops, int bdir, long long ext, char *out)
{
	if (n < 0 || n_ops < 0 || (n > 0 && (!cs || !out)) || (n_ops > 0 && !ops)) return -1;
	std::string o;
	gsah_cs_trim(cs, n, ops, n_ops, bdir, ext, o);
	if (o.size() > (size_t)n) return -2;
	if (!o.empty()) memcpy(out, o.data(), o.size());
	return (long long)o.size();
}

// The chain triples of every block of one finished contig (gsa_seg_block / gsa_seg, gsa_hip.h), on the host, from the gapped strings and seed records, untrimmed: what
// gsa_block_segs gives.  blk[res->n_blocks] is always filled; seg[cap]; returns the number of triples (call with cap = 0 to size `seg`), < 0 on error.  Needs no index.
long long gsah_c_segs(const gsa_result *res, gsa_seg_block *blk, gsa_seg *seg, long long cap)
{
	if (!res || (res->n_blocks > 0 && !blk) || (cap > 0 && !seg)) return -1;
	ContigResult cr; cr.assign(*res);
	std::vector<gsa_seg_block> b; std::vector<gsa_seg> o;
	gsah_block_segs(cr, b, o);
	if (!b.empty()) memcpy(blk, b.data(), b.size() * sizeof(gsa_seg_block));
	const size_t m = std::min<size_t>(o.size(), cap > 0 ? (size_t)cap : 0);
	if (m) memcpy(seg, o.data(), m * sizeof(gsa_seg));
	return (long long)o.size();
}

// gsah_segs_trim on one block's triples segs[n]: out[n] receives the triples that stay; returns their number
long long gsah_c_segs_trim(const gsa_seg *segs, long long n, int bdir, long long ext, gsa_seg *out)
{
	if (n < 0 || (n > 0 && (!segs || !out))) return -1;
	std::vector<gsa_seg> o;
	gsah_segs_trim(segs, n, bdir, ext, o);
	if (o.size() > (size_t)n) return -2;
	if (!o.empty()) memcpy(out, o.data(), o.size() * sizeof(gsa_seg));
	return (long long)o.size();
}

// gsah_lift through the C API: pos[n] lifted through one finished contig, on the host -- what gsa_lift gives.  out[cap]; returns the number of hits (call with cap = 0 to
// size `out`), < 0 on error.  The index of the last prefix stays loaded, behind a lock, as in gsah_c_variants (only its sequence table is read).
long long gsah_c_lift(const char *index_prefix, const gsa_result *res, const int64_t *pos, long long n, gsa_lift_hit *out, long long cap)
{
	static std::mutex mu; static std::string have; static HostIndex *idx = nullptr;
	std::lock_guard<std::mutex> lock(mu);
	if (!index_prefix || !res || n < 0 || (n > 0 && !pos) || (cap > 0 && !out)) return -1;
	if (!idx || have != index_prefix) {
		delete idx; idx = new HostIndex; have.clear(); std::string e;
		if (!gsah_load_index(index_prefix, *idx, e)) { delete idx; idx = nullptr; return -2; }
		have = index_prefix;
	}
	ContigResult cr; cr.assign(*res);
	std::vector<gsa_lift_hit> h;
	gsah_lift(*idx, cr, pos, n, h);
	const size_t m = std::min<size_t>(h.size(), cap > 0 ? (size_t)cap : 0);
	if (m) memcpy(out, h.data(), m * sizeof(gsa_lift_hit));
	return (long long)h.size();
}

// gsah_lift_regions through the C API: the regions [beg[i], end[i]) lifted through one finished contig, on the host -- what gsa_lift_regions gives.  out[cap]; returns the
// number of hits (call with cap = 0 to size `out`), < 0 on error.  The index of the last prefix stays loaded, behind a lock, as in gsah_c_lift (only its sequence table is read).
long long gsah_c_lift_regions(const char *index_prefix, const gsa_result *res, const int64_t *beg, const int64_t *end, long long n, gsa_region_hit *out, long long cap)
{
	static std::mutex mu; static std::string have; static HostIndex *idx = nullptr;
	std::lock_guard<std::mutex> lock(mu);
	if (!index_prefix || !res || n < 0 || (n > 0 && (!beg || !end)) || (cap > 0 && !out)) return -1;
	if (!idx || have != index_prefix) {
		delete idx; idx = new HostIndex; have.clear(); std::string e;
		if (!gsah_load_index(index_prefix, *idx, e)) { delete idx; idx = nullptr; return -2; }
		have = index_prefix;
	}
	ContigResult cr; cr.assign(*res);
	std::vector<gsa_region_hit> h;
	gsah_lift_regions(*idx, cr, beg, end, n, h);
	const size_t m = std::min<size_t>(h.size(), cap > 0 ? (size_t)cap : 0);
	if (m) memcpy(out, h.data(), m * sizeof(gsa_region_hit));
	return (long long)h.size();
}

// gsah_track through the C API: the per-window track of one finished contig at window length W, on the host -- what gsa_ref_track gives.  out[cap]; returns the number
// of windows (call with cap = 0 to size `out`), < 0 on error.  The index of the last prefix stays loaded, behind a lock, as in gsah_c_lift (only its sequence table is read).
long long gsah_c_track(const char *index_prefix, const gsa_result *res, int32_t W, gsa_track_win *out, long long cap)
{
	static std::mutex mu; static std::string have; static HostIndex *idx = nullptr;
	std::lock_guard<std::mutex> lock(mu);
	if (!index_prefix || !res || W < 1 || (cap > 0 && !out)) return -1;
	if (!idx || have != index_prefix) {
		delete idx; idx = new HostIndex; have.clear(); std::string e;
		if (!gsah_load_index(index_prefix, *idx, e)) { delete idx; idx = nullptr; return -2; }
		have = index_prefix;
	}
	ContigResult cr; cr.assign(*res);
	std::vector<gsa_track_win> w;
	gsah_track(*idx, cr, W, w);
	const size_t m = std::min<size_t>(w.size(), cap > 0 ? (size_t)cap : 0);
	if (m) memcpy(out, w.data(), m * sizeof(gsa_track_win));
	return (long long)w.size();
}

// gsah_qtrack through the C API: the per-window track of one finished contig of qlen bases over the query contig at window length W, on the host -- what
// gsa_query_track gives.  out[cap]; returns the number of windows (call with cap = 0 to size `out`), < 0 on error.  The index of the last prefix stays loaded, behind a
// lock, as in gsah_c_lift (only its sequence table is read: the trim).
long long gsah_c_qtrack(const char *index_prefix, const gsa_result *res, int32_t qlen, int32_t W, gsa_qtrack_win *out, long long cap)
{
	static std::mutex mu; static std::string have; static HostIndex *idx = nullptr;
	std::lock_guard<std::mutex> lock(mu);
	if (!index_prefix || !res || W < 1 || qlen < 0 || (cap > 0 && !out)) return -1;
	if (!idx || have != index_prefix) {
		delete idx; idx = new HostIndex; have.clear(); std::string e;
		if (!gsah_load_index(index_prefix, *idx, e)) { delete idx; idx = nullptr; return -2; }
		have = index_prefix;
	}
	ContigResult cr; cr.assign(*res);
	std::vector<gsa_qtrack_win> w;
	gsah_qtrack(*idx, cr, qlen, W, w);
	const size_t m = std::min<size_t>(w.size(), cap > 0 ? (size_t)cap : 0);
	if (m) memcpy(out, w.data(), m * sizeof(gsa_qtrack_win));
	return (long long)w.size();
}

// gsah_project through the C API: one finished contig painted into words[n_words] (n_words = G of the index), on the host -- what gsa_project paints.  seq: the query
// contig (its bases stand in the seeds' columns).  stat may be NULL.  Returns 0, < 0 on error (-3: n_words is not the reference's length).  The index of the last
// prefix stays loaded, behind a lock, as in gsah_c_lift (only its sequence table is read).
int gsah_c_project(const char *index_prefix, const char *seq, const gsa_result *res, uint32_t flags, uint32_t *words, long long n_words, gsa_proj_stat *stat)
{
	static std::mutex mu; static std::string have; static HostIndex *idx = nullptr;
	std::lock_guard<std::mutex> lock(mu);
	if (!index_prefix || !res || !words || (flags & ~(uint32_t)GSA_PROJ_NO_DUP)) return -1;
	if (!idx || have != index_prefix) {
		delete idx; idx = new HostIndex; have.clear(); std::string e;
		if (!gsah_load_index(index_prefix, *idx, e)) { delete idx; idx = nullptr; return -2; }
		have = index_prefix;
	}
	if (n_words != idx->G) return -3;
	ContigResult cr; cr.assign(*res);
	gsah_project(*idx, seq, cr, flags, words, stat);
	return 0;
}
// gsah_proj_text through the C API
int gsah_c_proj_text(const uint32_t *words, long long n, char *text)
{
	if (n < 0 || (n > 0 && (!words || !text))) return -1;
	gsah_proj_text(words, n, text);
	return 0;
}
// Emitter::proj_text through the C API: the FASTA text of words[G] for every sequence of the index, as -proj writes it.  out[cap]; returns the number of bytes (call with
// cap = 0 to size `out`), < 0 on error.
long long gsah_c_emit_proj(const char *index_prefix, const uint32_t *words, long long n_words, char *out, long long cap)
{
	std::string e; HostIndex idx;
	if (!index_prefix || !words || (cap > 0 && !out)) return -1;
	if (!gsah_load_index(index_prefix, idx, e)) return -2;
	if (n_words != idx.G) return -3;
	Emitter em; em.idx = &idx;
	std::string all, text;
	for (size_t c = 0; c < idx.chr_name.size(); c++) {
		text.resize((size_t)idx.chr_len[c]);
		gsah_proj_text(words + idx.chr_fwd[c], idx.chr_len[c], &text[0]);
		em.proj_text((int)c, text.data(), [&](OutBuf &&o) { all.append(o.p, o.n); });
	}
	const size_t m = std::min<size_t>(all.size(), cap > 0 ? (size_t)cap : 0);
	if (m) memcpy(out, all.data(), m);
	return (long long)all.size();
}

// OutputDotplot for one contig: script + data files (no gnuplot run).  Returns 1 if something was written.
// The reference plots AFTER OutputMAF (GSAlign.cpp:543-546), which shortens the last record of a block that runs over the end of
// its reference sequence (tools.cpp:149-220), and the plot shows the shortened block: the MAF emitter runs first here too.
int gsah_c_dotplot(const char *index_prefix, const char *query_fa, int contig, const char *gp_path, const char *out_prefix, gsah_result_cb cb, void *user, char *err)
{
	std::string e; HostIndex idx; std::vector<QueryContig> qs;
	if (!gsah_load_index(index_prefix, idx, e) || !gsah_load_query(query_fa, qs, e) || contig < 0 || contig >= (int)qs.size()) { if (err) { strncpy(err, e.c_str(), 255); err[255] = 0; } return -1; }
	gsa_result res; memset(&res, 0, sizeof(res));
	if (cb(user, contig, qs[(size_t)contig].seq.data(), (int)qs[(size_t)contig].seq.size(), &res) != 0) return -2;
	ContigResult cr; cr.assign(res);
	Emitter em; em.idx = &idx;
	if (!cr.blocks.empty()) { FILE *nul = fopen("/dev/null", "w"); if (nul) { em.maf(nul, false, qs[(size_t)contig], cr); fclose(nul); } }
	return em.dotplot(gp_path, out_prefix, qs[(size_t)contig], cr) ? 1 : 0;
}

} // extern "C"
