// gsalign_amd/csrc/host/gsa_host.h -- CPU-side parts of the aligner that
// north_star keeps on the host: index build/load, query FASTA loading, MAF / ALN
// / VCF emission.  Plain C++ (g++), no HIP.  Built twice: into the CLI
// (GSAlign_hip) and into libgsa_host.so, whose C entry points let the CPU tests
// drive the emitters and the index builder without a GPU.
#ifndef GSA_HOST_H
#define GSA_HOST_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <functional>
#include <string>
#include <vector>
#include "gsa_hip.h"

// A buffer that is NOT zero-filled when it is sized: the index arrays of a 3.08 Gbp reference are 11 GB that the loader overwrites anyway
// (std::vector / std::string would first clear them on one thread, ~1 s; the loader's threads then fault the pages in themselves).
template <class T> struct RawBuf {
	T *p = nullptr; size_t n = 0;
	RawBuf() {}
	RawBuf(const RawBuf &) = delete; RawBuf &operator=(const RawBuf &) = delete;
	~RawBuf() { free(p); }
	void resize(size_t m) { free(p); p = m ? (T *)malloc(m * sizeof(T)) : nullptr; n = p ? m : 0; }
	T *data() { return p; } const T *data() const { return p; }
	size_t size() const { return n; }
	T &operator[](size_t i) { return p[i]; } const T &operator[](size_t i) const { return p[i]; }
};

struct HostIndex {
	uint64_t primary = 0, L2[5] = {0, 0, 0, 0, 0};
	RawBuf<uint32_t> bwt;
	RawBuf<uint64_t> sa;
	int64_t G = 0;
	std::vector<std::string> chr_name;
	std::vector<int32_t> chr_len;
	std::vector<int64_t> chr_fwd, chr_rev;        // FowardLocation / ReverseLocation (bwt_index.cpp:247-248)
	std::vector<int64_t> end_key; std::vector<int32_t> end_chr;   // ChrLocMap as sorted arrays
	RawBuf<char> ref;                             // RefSequence: 2G ASCII
	RawBuf<uint8_t> pac;                          // the .pac bytes (between gsah_load_index_files and gsah_unpack_ref)

	void fill_view(gsa_index_view *v) const;
	// GenCoordinateInfo (tools.cpp:120-140)
	void coordinate(int64_t rpos, int *bdir, int *chr, int *gpos) const;
};

struct QueryContig { std::string name, seq; };

// index files (reference src/bwt_index.cpp:25-264, src/GetData.cpp:8-24)
bool gsah_index_files_exist(const std::string &prefix);
bool gsah_load_index(const std::string &prefix, HostIndex &idx, std::string &err);
// the same in two steps: the files as they are (idx.pac = the raw .pac bytes, idx.ref still empty), then RestoreReferenceInfo's unpacking (bwt_index.cpp:229-264) --
// a host hands idx.pac to gsa_create_opts(GSA_CREATE_REF_PAC) after the first step and unpacks its own RefSequence while the device builds its tables
bool gsah_load_index_files(const std::string &prefix, HostIndex &idx, std::string &err);
bool gsah_unpack_ref(HostIndex &idx, std::string &err, bool keep_pac = false);
// bwa_idx_build (reference src/BWT_Index/bwtindex.c:77-149): byte-identical .bwt .sa .pac .ann .amb
bool gsah_build_index(const std::string &fasta, const std::string &prefix, std::string &err);
// The same with the BWT/SA half supplied by the caller: fn(user, pac, G, &primary, L2, bwt, sa) gets the .pac bytes of the G forward bases and fills primary, L2[0..4]
// (L2[0] = 0, L2[4] = 2G), the interleaved bwt words and the sampled SA (sa[0] = -1) -- the arrays of gsa_index_view, sized as gsa_index_sizes says -- and returns 0;
// anything else fails the build before .bwt / .sa are written.  fn = nullptr: the host's own suffix sorters, i.e. gsah_build_index.  gsa_build_index (gsa_hip.h) has
// this shape behind a device ordinal; this library links no HIP.
typedef int (*gsah_bwt_fn)(void *user, const uint8_t *pac, int64_t G, uint64_t *primary, uint64_t L2[5], uint32_t *bwt, uint64_t *sa);
bool gsah_build_index_with(const std::string &fasta, const std::string &prefix, std::string &err, gsah_bwt_fn fn, void *user);
// The reference half of an index WITHOUT the index: the builder's FASTA pass (read_fasta, srand48(11) / lrand48 for ambiguous bases, the .pac packing) into idx -- G, chr_name
// (as the .ann round trip delivers them), chr_len, chr_fwd / chr_rev, end_key / end_chr and idx.pac = the ceil(G / 4) .pac bytes; bwt / sa / ref stay empty.  Touches no
// file but the FASTA.  idx.pac goes to gsa_create_from_pac (gsa_hip.h), gsah_unpack_ref gives the emitters their RefSequence as after gsah_load_index_files.
bool gsah_reference_from_fasta(const std::string &fasta, HostIndex &idx, std::string &err);
// LoadQueryFile / TrimChromosomeName / CheckQuerySeq (reference src/main.cpp:35-114)
bool gsah_load_query(const std::string &path, std::vector<QueryContig> &out, std::string &err);

// A plain array that is allocated WITHOUT being touched (std::vector / std::string write every byte once before the copy does, or fault their pages on one
// thread): a 250 Mb contig's records and gapped strings are ~150 MB, and a GPU worker thread is inside the result callback while they are copied.
template <class T> struct RawArr {
	T *p = nullptr; size_t n = 0;
	RawArr() {}
	RawArr(const RawArr &) = delete; RawArr &operator=(const RawArr &) = delete;
	RawArr(RawArr &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
	RawArr &operator=(RawArr &&o) noexcept { if (this != &o) { free(p); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
	~RawArr() { free(p); }
	void reset() { free(p); p = nullptr; n = 0; }
	void assign(const T *src, size_t count);            // emit.cpp: large arrays are copied by the pool's threads (first touch spread over them)
	T *data() { return p; } const T *data() const { return p; }
	size_t size() const { return n; }
	T &operator[](size_t i) { return p[i]; } const T &operator[](size_t i) const { return p[i]; }
};

// one finished contig, as delivered by gsa_align_contig
struct ContigResult {
	std::vector<gsa_block> blocks;
	RawArr<gsa_rec> recs;                  // the 16-byte records as they arrived; frag(i) is record i as a FragPair_t
	RawArr<char> aln1, aln2;
	bool summary = false;                  // a summary result: recs = the block ends, recs[2b] / recs[2b + 1] the first / last record of block b; no strings
	void assign(const gsa_result &r, bool summary_mode = false);      // the copies only: what a GPU worker thread does inside the result callback (aln1 == NULL with n_aln == 0 is fine)
	gsa_frag frag(int64_t i) const { gsa_frag f; gsa_rec_expand(recs.data(), i, &f); return f; }
	void trim(int64_t i, int ext);         // iExtension (tools.cpp:192-202): record i loses its last `ext` bases
};

// Variant_t (structure.h:124-132); the two alleles are pieces of RefSequence / of the query sequence and are pointed at, not copied:
// both outlive the Emitter's list (the index and the query contigs are loaded once per run)
struct Variant { int pos, chr_idx, query_idx, type; const char *ref_p, *alt_p; uint32_t ref_n, alt_n; };

// VariantIdentification as gsa_variant records (emit.cpp): the host walk in the layout and order of gsa_call_variants
int64_t gsah_variant_records(const HostIndex *idx, const ContigResult &r, gsa_variant *out, int64_t cap, int64_t counts[3]);

// The CIGAR of every block of a finished contig (gsa_block_cigar / ops as in gsa_hip.h), computed from the gapped strings and the seed records themselves,
// UNTRIMMED: what gsa_block_cigars computes on the device from op strings -- its comparator, and the CIGAR source of a host that holds a gsa_result and no GPU
// context.  seq (may be NULL) = the query contig: a seed's columns are then classified from its text like any other column, else taken as '='.
void gsah_block_cigars(const char *seq, const ContigResult &r, std::vector<gsa_block_cigar> &blk, std::vector<uint32_t> &ops);
// iExtension's trim (tools.cpp:192-202) on a block's ops: the last `ext` columns IN WALK ORDER go -- the last ops of a forward block, the FIRST ones of a
// reverse-strand block (its ops are in output order).  out = the ops that stay; bc's op count and columns per class are reduced by what was removed.
void gsah_cigar_trim(const uint32_t *ops, int bdir, int64_t ext, std::vector<uint32_t> &out, gsa_block_cigar &bc);
// The cs string of every block of a finished contig (gsa_cs_block / bytes as in gsa_hip.h), UNTRIMMED: the walk of gsah_block_cigars over the records and the two
// gapped strings that also writes the tokens -- the comparator of gsa_block_cs.  It needs only the strings: a seed is ":len".
void gsah_block_cs(const ContigResult &r, std::vector<gsa_cs_block> &blk, std::string &cs);
// iExtension's trim on ONE block's cs string (cs[n], the string of the block's untrimmed ops[n_ops], output order): the columns gsah_cigar_trim drops go -- the
// tail of a forward block's string, the head of a reverse-strand block's -- and a cut ":n" is printed again.  out = the cs of the trimmed ops.
void gsah_cs_trim(const char *cs, int64_t n, const uint32_t *ops, int64_t n_ops, int bdir, int64_t ext, std::string &out);

// The chain triples of every block of a finished contig (gsa_seg_block / gsa_seg as in gsa_hip.h), UNTRIMMED: the column walk of gsah_block_cigars over the records
// and the two gapped strings with a merge of its own -- a state machine over aligned / gap columns, no CIGAR ops in between.  The comparator of gsa_block_segs, and the
// chain source of a host that holds a gsa_result and no GPU context.
void gsah_block_segs(const ContigResult &r, std::vector<gsa_seg_block> &blk, std::vector<gsa_seg> &segs);
// iExtension's trim on ONE block's triples (segs[n], output order): the last `ext` columns IN WALK ORDER go -- they are taken off the last triples of a forward block,
// off the FIRST ones of a reverse-strand block.  A cut that falls inside a gap or at its edge takes the whole gap: a chain neither starts nor ends with one.  out = the
// triples that stay (the last one with dt = dq = 0; empty when nothing stays).  Needs only the triples.
void gsah_segs_trim(const gsa_seg *segs, int64_t n, int bdir, int64_t ext, std::vector<gsa_seg> &out);

// The positions pos[0 .. n) (0-based forward global reference coordinates) lifted through a finished contig, by the contract of gsa_lift (gsa_hip.h): coverage trimmed by
// iExtension, the choice among covering blocks, the class and query position of the chosen column -- from the records and the two gapped strings.  The comparator of
// gsa_lift, and the lift of a host that holds a gsa_result and no GPU context.  hits: ascending in idx, positions no block covers (or outside [0, G)) absent.
void gsah_lift(const HostIndex &ix, const ContigResult &r, const int64_t *pos, int64_t n, std::vector<gsa_lift_hit> &hits);

// The regions [beg[i], end[i]) (0-based forward global reference coordinates, half-open) lifted through a finished contig, by the contract of gsa_lift_regions (gsa_hip.h):
// trimmed coverage, the choice among overlapping blocks (overlap before score), the span's four class counts and its query interval -- from the records and the two gapped
// strings, column by column.  The comparator of gsa_lift_regions, and the interval lift of a host that holds a gsa_result and no GPU context.  hits: ascending in idx,
// regions no block overlaps (or that are empty, outside [0, G) or across a sequence boundary) absent.
void gsah_lift_regions(const HostIndex &ix, const ContigResult &r, const int64_t *beg, const int64_t *end, int64_t n, std::vector<gsa_region_hit> &hits);

// The per-window track of a finished contig over the reference sequences at window length W, by the contract of gsa_ref_track (gsa_hip.h): counted blocks, trimmed
// coverage, column classes, the insertion rule -- from the records and the two gapped strings.  The comparator of gsa_ref_track, and the track of a host that holds a
// gsa_result and no GPU context.  win: one record per window with n_cov > 0, ascending by (chr, start); empty for a summary result or W <= 0.
void gsah_track(const HostIndex &ix, const ContigResult &r, int32_t W, std::vector<gsa_track_win> &win);
// The per-window track of a finished contig of qlen bases over the QUERY contig at window length W, by the contract of gsa_query_track (gsa_hip.h): counted blocks, the
// trim carried over from the reference side, column classes, the deletion rule, union and multi coverage -- from the records and the two gapped strings.  The
// comparator of gsa_query_track.  win: one record per window with n_cov > 0, ascending by start; empty for a summary result, W <= 0 or qlen <= 0.
void gsah_qtrack(const HostIndex &ix, const ContigResult &r, int32_t qlen, int32_t W, std::vector<gsa_qtrack_win> &win);

// A finished contig painted into the caller's accumulator words[0 .. G) by the contract of gsa_project (gsa_hip.h): trimmed coverage, the CIGAR pass's columns, key | code,
// the maximum stays (taken atomically: several threads may meet in a word) -- from the records, the two gapped strings and, for the seeds, the query contig seq (NULL: a
// seed's bases count as 'N').  flags: GSA_PROJ_NO_DUP.  The comparator of gsa_project, and the projection of a host that holds a gsa_result and no GPU context.
void gsah_project(const HostIndex &ix, const char *seq, const ContigResult &r, uint32_t flags, uint32_t *words, gsa_proj_stat *stat = nullptr);
// words -> characters (codes 1..6: A C G T N -, word 0: n), n of them, no NUL
void gsah_proj_text(const uint32_t *words, int64_t n, char *text);

struct OutBuf;                             // par.h

struct Emitter {
	const HostIndex *idx = nullptr;
	bool allow_dup = true;                 // !-unique
	std::vector<Variant> vars;             // VarVec ...
	std::vector<std::vector<Variant> > var_chunks;   // ... kept as the lists the pool's threads filled, in the serial order (vars first)
	int n_snv = 0, n_ins = 0, n_del = 0;
	// OutputMAF (tools.cpp:149-220).  first = (QueryChrIdx == 0).  May shorten the last record of a block (iExtension).
	void maf(FILE *fp, bool first, const QueryContig &q, ContigResult &r) const;
	// the same bytes handed to `sink` buffer after buffer, in order; a block's two text lines are filled by the pool's threads (par.h);
	// `take(n)` supplies the large buffers (OrderedWriter::take recycles them)
	void maf_text(bool first, const QueryContig &q, ContigResult &r, const std::function<void(OutBuf &&)> &sink, const std::function<OutBuf(size_t)> &take) const;
	void maf_block(const QueryContig &q, ContigResult &r, gsa_block &b, OutBuf &small, const std::function<void(OutBuf &&)> &sink, const std::function<OutBuf(size_t)> &take) const;
	// PAF: one line per block with its cg:Z: CIGAR, blocks selected and trimmed (iExtension) like OutputMAF's; blk / ops = the contig's CIGARs from gsa_block_cigars,
	// or NULL: computed here (gsah_block_cigars).  Shortens the last record of a block exactly as maf_block does.  A summary result (ContigResult::summary) must
	// bring its CIGARs: the first and last record of block bi are recs[2 bi] and recs[2 bi + 1], and no string is touched.
	// csb / cs (optional; they need blk / ops) = the contig's cs strings from gsa_block_cs: every line gets "\tcs:Z:<string>" behind its cg:Z: field, trimmed like the ops.
	void paf_text(const QueryContig &q, ContigResult &r, const gsa_block_cigar *blk, const uint32_t *ops, const std::function<void(OutBuf &&)> &sink,
	              const gsa_cs_block *csb = nullptr, const char *cs = nullptr) const;
	void paf(FILE *fp, const QueryContig &q, ContigResult &r, const gsa_block_cigar *blk, const uint32_t *ops, const gsa_cs_block *csb = nullptr, const char *cs = nullptr) const;
	// <prefix>.lift.tsv (-lift): one line per hit of gsa_lift / gsah_lift, in the order given -- reference name, 1-based position, query name, 1-based query position, + / -,
	// class letter (= X D), the block's score as the MAF prints it (1 for a duplicate), n_cover; first: the header line in front.  ref_chr / ref_pos: reference sequence
	// and 1-based position of every input position (gsa_lift_hit::idx indexes them)
	void lift_text(bool first, const QueryContig &q, const ContigResult &r, const gsa_lift_hit *hits, int64_t n_hits, const int32_t *ref_chr, const int32_t *ref_pos,
	               const std::function<void(OutBuf &&)> &sink) const;
	// <prefix>.regions.tsv (-liftbed): one line per hit of gsa_lift_regions / gsah_lift_regions, in the order given -- reference name, the region's start and end (BED-style:
	// 0-based, half-open, inside the sequence), its name, the covered part's start and end, query name, the query interval (0-based, half-open, in the contig as stored),
	// + / -, match, mismatch, deleted, inserted, the block's score as the MAF prints it (1 for a duplicate), n_cover; first: the header line in front.  ref_chr / ref_beg /
	// ref_end / name: sequence, local interval and name of every input region (gsa_region_hit::idx indexes them)
	void regions_text(bool first, const QueryContig &q, const ContigResult &r, const gsa_region_hit *hits, int64_t n_hits, const int32_t *ref_chr, const int32_t *ref_beg,
	                  const int32_t *ref_end, const std::string *name, const std::function<void(OutBuf &&)> &sink) const;
	// <prefix>.track.tsv (-track W): one line per window of gsa_ref_track / gsah_track, in the order given -- reference name, start and end (BED-style: 0-based, half-open,
	// inside the sequence), query name, covered, match, mismatch, deleted, inserted; first: the header line in front
	void track_text(bool first, const QueryContig &q, const gsa_track_win *win, int64_t n_win, const std::function<void(OutBuf &&)> &sink) const;
	// <prefix>.qtrack.tsv (-qtrack W): one line per window of gsa_query_track / gsah_qtrack, in the order given -- query name, start and end (BED-style) inside the
	// contig, covered, multi, match, mismatch, inserted, deleted; first: the header line in front
	void qtrack_text(bool first, const QueryContig &q, const gsa_qtrack_win *win, int64_t n_win, const std::function<void(OutBuf &&)> &sink) const;
	// <prefix>.chain (-chain): a UCSC chain per block, blocks selected like OutputMAF's (-unique), from the block's UNTRIMMED triples blk / seg (gsa_block_segs; NULL: computed
	// here, gsah_block_segs) cut by iExtension (gsah_segs_trim) --
	//   chain <score> <tName> <tSize> + <tStart> <tEnd> <qName> <qSize> <+|-> <qStart> <qEnd> <id> / "size dt dq" per triple but the last / "size" / an empty line
	// score as the MAF prints it (trimmed; 1 for a duplicate); coordinates 0-based, half-open, for '-' on the query's reverse strand (the MAF `s` line's convention), and
	// tEnd - tStart = sum(size + dt), qEnd - qStart = sum(size + dq).  A forward block starts where its MAF line starts; a reverse-strand block starts where its MAF line
	// starts (the end of its last record, shortened by the `ext` columns as the MAF shortens it) moved on by the bases of the gap columns the trim left at that edge,
	// which go with their gap.  *id: the last id given (the file's ids count from 1 in output order); a block left without a
	// segment prints nothing and takes none.  r is not changed: the trim is read off the untrimmed last record, so the call goes IN FRONT of maf_text / paf_text / aln,
	// which shorten it -- once.
	void chain_text(const QueryContig &q, const ContigResult &r, const gsa_seg_block *blk, const gsa_seg *seg, int64_t *id, const std::function<void(OutBuf &&)> &sink) const;
	void chain(FILE *fp, const QueryContig &q, const ContigResult &r, const gsa_seg_block *blk, const gsa_seg *seg, int64_t *id) const;
	// <prefix>.proj.fa (-proj): one FASTA record of the projected query -- '>' and reference sequence `chr`'s name as the .ann round trip delivers it, then its characters
	// text[0 .. chr_len) (gsa_proj_fetch / gsah_proj_text of the sequence's positions), 60 per line
	void proj_text(int chr, const char *text, const std::function<void(OutBuf &&)> &sink) const;
	// OutputAlignment (tools.cpp:222-286)
	void aln(FILE *fp, const QueryContig &q, ContigResult &r) const;
	// OutputDotplot (DotPloting.cpp:10-71): gnuplot script `gp_path` + one data file per plotted reference sequence
	// (`<prefix>.<query>vs<chr>`); returns false when there is nothing to plot.  Running gnuplot on the script and removing
	// the data files afterwards (DotPloting.cpp:69-70) is the caller's business: `data_files` receives their names.
	bool dotplot(const std::string &gp_path, const std::string &out_prefix, const QueryContig &q, const ContigResult &r, std::vector<std::string> *data_files = nullptr) const;
	// VariantIdentification (SeqVariant.cpp:12-119); long blocks are dealt to the pool in record ranges
	void variants(int query_idx, const QueryContig &q, ContigResult &r);
	// the same list from the records of gsa_call_variants (the walk ran on the GPU): n variants of contig `query_idx`, in their serial order
	void variants_from(int query_idx, const QueryContig &q, const gsa_variant *v, int64_t n);
	// OutputSequenceVariants (SeqVariant.cpp:121-143)
	void vcf(FILE *fp, const std::string &reference_label);
	void vcf_text(const std::string &reference_label, const std::function<void(OutBuf &&)> &sink);
};

#endif
