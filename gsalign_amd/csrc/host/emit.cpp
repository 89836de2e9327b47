// gsalign_amd/csrc/host/emit.cpp -- query FASTA loader and the MAF / ALN / VCF
// emitters.  CPU code by design (north_star keeps MAF/VCF emission on the host).
//
// Follows, quirk for quirk (SURVEY.md App. A.7, App. B #4,#15-#21):
//   LoadQueryFile / TrimChromosomeName / CheckQuerySeq   reference src/main.cpp:35-114
//   OutputMAF / OutputAlignment / SelfComplementarySeq   src/tools.cpp:3-44,149-286
//   VariantIdentification / OutputSequenceVariants       src/SeqVariant.cpp:6-143
#include <algorithm>
#include <array>
#include <atomic>
#include <cstring>
#include <fstream>
#include <memory>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include "gsa_host.h"
#include "par.h"
#include "exact_sort.h"

namespace {

// blocks / lists / files below this size are handled by the calling thread alone.  GSA_HOST_PAR_MIN (read at every call: the CPU tests switch it)
// forces the parallel forms on the small goldens
size_t par_min_bytes() { const char *e = getenv("GSA_HOST_PAR_MIN"); return e ? (size_t)atoll(e) : (size_t)1 << 20; }

inline int nt4(unsigned char c)
{
	switch (c | 0x20) { case 'a': return 0; case 'c': return 1; case 'g': return 2; case 't': return 3; default: return 4; }
}

// tools.cpp:3-31: ACGTN/acgtn -> upper-case complement, U/u -> A, '-' stays, everything else NUL
inline char rev_map(char c)
{
	switch (c) {
	case 'A': case 'a': return 'T'; case 'C': case 'c': return 'G'; case 'G': case 'g': return 'C'; case 'T': case 't': return 'A';
	case 'U': case 'u': return 'A'; case 'N': case 'n': return 'N'; case '-': return '-';
	default: return '\0';
	}
}

// TrimChromosomeName (main.cpp:35-47): '|' -> '-', cut at space # : = tab
std::string trim_name(const char *p, size_t n)
{
	std::string name(p, n); size_t i;
	for (i = 0; i < name.size(); i++) {
		if (name[i] == '|') name[i] = '-';
		else if (name[i] == ' ' || name[i] == '#' || name[i] == ':' || name[i] == '=' || name[i] == '\t') break;
	}
	return name.substr(0, i);
}

int count_gaps(const std::string &s, int i, int stop) { int n = 0; for (; i < stop; i++) if (s[i] == '-') n++; return n; }

// the two text lines of a block, built exactly like OutputMAF does (tools.cpp:168-184)
void block_text(const QueryContig &q, const ContigResult &r, const gsa_block &b, std::string &t1, std::string &t2)
{
	t1.clear(); t2.clear();
	for (int k = 0; k < b.n_frag; k++) {
		const gsa_frag f = r.frag(b.frag_off + k);
		if (f.bseed) { t1.append(q.seq, f.qpos, f.qlen); t2.append(q.seq, f.qpos, f.qlen); }     // seeds print the QUERY text on both lines (App. B #4)
		else { t1.append(r.aln1.data() + f.aln_off, (size_t)f.aln_len); t2.append(r.aln2.data() + f.aln_off, (size_t)f.aln_len); }
	}
}

// iExtension (tools.cpp:192-202): a block running past the end of its chromosome copy is trimmed
int extension(const HostIndex &ix, const gsa_block &b, const gsa_frag &last)
{
	const int64_t end = last.rpos + last.rlen;
	const int64_t lim = (b.bdir ? ix.chr_fwd[b.chr] : ix.chr_rev[b.chr]) + ix.chr_len[b.chr];
	return end > lim ? (int)(end - lim) : 0;
}

} // namespace

// what a GPU worker thread does inside gsa_align_many's callback: the result is valid during the call only, so its bytes are copied -- and
// nothing else.  The records stay in their 16-byte form: the emitters expand the one they look at (frag()), 70 M records of a human genome
// are never materialised as 40-byte FragPair_t copies

template <class T> void RawArr<T>::assign(const T *src, size_t count)
{
	reset();
	if (count == 0) return;
	p = (T *)malloc(count * sizeof(T)); if (!p) abort();
	n = count;
	const size_t bytes = count * sizeof(T);
	char *d = (char *)p; const char *sp = (const char *)src;
	if (bytes < ((size_t)8 << 20)) { memcpy(d, sp, bytes); return; }
	par_ranges(bytes, (size_t)2 << 20, [&](size_t b, size_t e) { memcpy(d + b, sp + b, e - b); });
}
template struct RawArr<gsa_rec>;
template struct RawArr<char>;
template struct RawArr<gsa_variant>;
template struct RawArr<gsa_block_cigar>;
template struct RawArr<gsa_cs_block>;
template struct RawArr<uint32_t>;
template struct RawArr<gsa_lift_hit>;
template struct RawArr<gsa_region_hit>;
template struct RawArr<gsa_track_win>;
template struct RawArr<gsa_qtrack_win>;
template struct RawArr<gsa_seg_block>;
template struct RawArr<gsa_seg>;
void ContigResult::assign(const gsa_result &r, bool summary_mode)
{
	summary = summary_mode;
	blocks.assign(r.blocks, r.blocks + r.n_blocks);
	recs.assign(r.recs, (size_t)r.n_frags);
	aln1.assign(r.aln1, (size_t)r.n_aln); aln2.assign(r.aln2, (size_t)r.n_aln);
}

// iExtension's trim of a block's last record (tools.cpp:192-202): a seed's one length, or a gap's two
void ContigResult::trim(int64_t i, int ext)
{
	gsa_rec &x = recs[(size_t)i];
	// A block's records are seed [gap] seed ... seed (gsa_hip.h): the last one is a seed, whose tag is its qpos -- its length may go to
	// zero or below exactly as the reference's qLen / rLen do.  A gap's tag is the SIGN of nqlen (= -1 - qLen): it never crosses zero here,
	// so a record can not change its kind under a later gsa_rec_expand.
	if (x.seed.qpos >= 0) x.seed.len -= ext;
	else { x.gap.rlen -= ext; x.gap.nqlen = (int64_t)x.gap.nqlen + ext > -1 ? -1 : x.gap.nqlen + ext; }
}

// LoadQueryFile (main.cpp:82-114) line by line -- getline on '\n', empty lines skipped, a line that starts with '>' opens a sequence
// (TrimChromosomeName), every other line loses ONE trailing '\r', must be all isalpha (CheckQuerySeq) and is appended -- but on the whole
// file at once: the file is read in slices by the pool's threads, cut into segments at line starts, every segment validates and counts
// its lines (pass 1), the sequences get their sizes, every segment copies its lines to where they belong (pass 2).  3 GB of FASTA: the
// reference's getline loop takes ~10 s, this takes the time of two passes over the page cache.
bool gsah_load_query(const std::string &path, std::vector<QueryContig> &out, std::string &err)
{
	const int fd = open(path.c_str(), O_RDONLY);
	if (fd < 0) { err = "cannot open " + path; return false; }
	struct stat st;
	if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
		// not a regular file (a pipe): the serial reader
		close(fd);
		std::ifstream file(path.c_str());
		if (!file.is_open()) { err = "cannot open " + path; return false; }
		std::string str; bool first = true;
		while (std::getline(file, str)) {
			if (first) { first = false; if (str.empty() || str[0] != '>') { err = "not a FASTA file: " + path; return false; } }
			if (str.empty()) continue;
			if (str[0] == '>') { QueryContig qc; qc.name = trim_name(str.data() + 1, str.size() - 1); out.push_back(qc); }
			else {
				if (str[str.size() - 1] == '\r') str.resize(str.size() - 1);
				for (size_t i = 0; i < str.size(); i++) if (!isalpha((unsigned char)str[i])) { err = "The query sequence contains non-alphabet characters!"; return false; }
				if (out.empty()) { err = "sequence before the first header"; return false; }
				out.back().seq.append(str);
			}
		}
		if (out.empty()) { err = "no sequence in " + path; return false; }
		return true;
	}
	const size_t n = (size_t)st.st_size;
	if (n == 0) { close(fd); err = "not a FASTA file: " + path; return false; }
	std::unique_ptr<char[]> buf(new char[n]);
	std::atomic<bool> io_ok(true);
	par_ranges(n, (size_t)8 << 20, [&](size_t b, size_t e) {
		while (b < e) { const ssize_t r = pread(fd, buf.get() + b, e - b, (off_t)b); if (r <= 0) { io_ok = false; return; } b += (size_t)r; }
	});
	close(fd);
	if (!io_ok) { err = "cannot read " + path; return false; }
	const char *d = buf.get();
	if (d[0] != '>') { err = "not a FASTA file: " + path; return false; }      // (the first line is empty or no header: CheckInputFile, main.cpp:49-64)
	// segments: [seg[k], seg[k + 1]) each starting at a line start
	const size_t want = std::min<size_t>((size_t)HostPool::global().threads() * 4, n / std::max<size_t>(par_min_bytes(), 1) + 1);
	std::vector<size_t> seg(1, 0);
	for (size_t k = 1; k < want; k++) {
		size_t p = n * k / want; if (p <= seg.back()) continue;
		const char *nl = (const char *)memchr(d + p, '\n', n - p);
		if (!nl) break;
		p = (size_t)(nl - d) + 1;
		if (p > seg.back() && p < n) seg.push_back(p);
	}
	seg.push_back(n);
	const size_t S = seg.size() - 1;
	struct Piece { size_t hdr_off, hdr_len; size_t bases; };         // a header line (hdr_len = 0 for the headless first piece of a segment) and the bases that follow it in the segment
	std::vector<std::vector<Piece> > pieces(S);
	std::atomic<bool> bad(false);
	static const struct AlphaTab { bool ok[256]; AlphaTab() { for (int c = 0; c < 256; c++) ok[c] = isalpha(c) != 0; } } alpha;
	// calls line(ptr, len) for every line of the segment (without its '\n')
	auto each_line = [&](size_t k, auto &&line) {
		size_t p = seg[k]; const size_t e = seg[k + 1];
		while (p < e) {
			const char *nl = (const char *)memchr(d + p, '\n', e - p);
			const size_t le = nl ? (size_t)(nl - d) : e;
			line(p, le - p);
			p = le + 1;
		}
	};
	HostPool::global().run(S, [&](size_t k) {
		std::vector<Piece> &pc = pieces[k];
		pc.push_back(Piece{ 0, 0, 0 });
		each_line(k, [&](size_t p, size_t len) {
			if (len == 0) return;
			if (d[p] == '>') { pc.push_back(Piece{ p, len, 0 }); return; }
			if (d[p + len - 1] == '\r') len--;
			bool ok = true;
			for (size_t i = 0; i < len; i++) ok &= alpha.ok[(unsigned char)d[p + i]];
			if (!ok) bad = true;
			pc.back().bases += len;
		});
	});
	if (bad) { err = "The query sequence contains non-alphabet characters!"; return false; }
	// sequences and the place of every piece in them
	const size_t base = out.size();                  // (a caller may hand in a vector that already holds contigs)
	std::vector<std::vector<size_t> > dst(S), cidx(S);
	std::vector<size_t> total;
	for (size_t k = 0; k < S; k++) {
		dst[k].assign(pieces[k].size(), 0); cidx[k].assign(pieces[k].size(), 0);
		for (size_t j = 0; j < pieces[k].size(); j++) {
			const Piece &pc = pieces[k][j];
			if (pc.hdr_len) { QueryContig qc; qc.name = trim_name(d + pc.hdr_off + 1, pc.hdr_len - 1); out.push_back(qc); total.push_back(0); }
			if (total.empty()) { if (pc.bases) { err = "sequence before the first header"; return false; } continue; }
			cidx[k][j] = total.size() - 1; dst[k][j] = total.back(); total.back() += pc.bases;
		}
	}
	if (total.empty()) { err = "no sequence in " + path; return false; }
	HostPool::global().run(total.size(), [&](size_t c) { out[base + c].seq.resize(total[c]); });
	HostPool::global().run(S, [&](size_t k) {
		size_t j = 0;
		char *w = pieces[k][0].bases ? &out[base + cidx[k][0]].seq[0] + dst[k][0] : nullptr;
		each_line(k, [&](size_t p, size_t len) {
			if (len == 0) return;
			if (d[p] == '>') { j++; w = pieces[k][j].bases ? &out[base + cidx[k][j]].seq[0] + dst[k][j] : nullptr; return; }
			if (d[p + len - 1] == '\r') len--;
			if (len) { memcpy(w, d + p, len); w += len; }
		});
	});
	return true;
}

// One block of OutputMAF (tools.cpp:164-216) as bytes.  The two text lines are filled piece by piece -- a seed prints the QUERY text on both
// lines, a gap its two gapped strings -- by the pool's threads, each piece at the offset the serial concatenation gives it; trimming
// (iExtension), the '-' counts, the reverse-complement of a reverse-strand block (SelfComplementarySeq: in place, pairs (i, L-1-i) are
// independent) and the NUL quirk (an unknown byte maps to '\0' and "%s" stops there) are the serial code's.
void Emitter::maf_block(const QueryContig &q, ContigResult &r, gsa_block &b, OutBuf &small, const std::function<void(OutBuf &&)> &sink, const std::function<OutBuf(size_t)> &take) const
{
	const int64_t f0 = b.frag_off;
	const size_t nf = (size_t)b.n_frag;
	std::vector<size_t> off(nf + 1); off[0] = 0;
	auto piece = [&](size_t lo, size_t hi) { for (size_t k = lo; k < hi; k++) { const gsa_frag f = r.frag(f0 + (int64_t)k); off[k + 1] = (size_t)(f.bseed ? f.qlen : f.aln_len); } };
	if (nf * 16 >= par_min_bytes()) par_ranges(nf, (size_t)1 << 16, piece); else piece(0, nf);
	for (size_t k = 0; k < nf; k++) off[k + 1] += off[k];
	const size_t total = off[nf];
	gsa_frag last = r.frag(f0 + (int64_t)nf - 1);
	const int ext = extension(*idx, b, last);
	if (ext > 0) { b.aln_len -= ext; b.score -= ext; last.rlen -= ext; last.qlen -= ext; r.trim(f0 + (int64_t)nf - 1, ext); }
	const size_t L = (size_t)(b.aln_len > 0 ? b.aln_len : 0);
	const bool big = 2 * L >= par_min_bytes();
	OutBuf t1 = big ? take(L + 1) : OutBuf(L + 1), t2 = big ? take(L + 1) : OutBuf(L + 1);
	const size_t fillable = total < L ? total : L;
	auto fill = [&](size_t pb, size_t pe) {      // text positions [pb, pe)
		size_t k = (size_t)(std::upper_bound(off.begin(), off.end(), pb) - off.begin()) - 1;
		for (size_t p = pb; p < pe; k++) {
			const size_t o = p - off[k], n = std::min(off[k + 1], pe) - p;
			if (n == 0) continue;
			const gsa_frag f = r.frag(f0 + (int64_t)k);
			if (f.bseed) { memcpy(t1.p + p, q.seq.data() + f.qpos + o, n); memcpy(t2.p + p, q.seq.data() + f.qpos + o, n); }
			else { memcpy(t1.p + p, r.aln1.data() + f.aln_off + o, n); memcpy(t2.p + p, r.aln2.data() + f.aln_off + o, n); }
			p += n;
		}
	};
	std::atomic<long long> g1(0), g2(0);
	auto gaps = [&](size_t pb, size_t pe) { long long a = 0, c = 0; for (size_t i = pb; i < pe; i++) { a += t1.p[i] == '-'; c += t2.p[i] == '-'; } g1 += a; g2 += c; };
	auto revpair = [&](char *s, size_t ib, size_t ie) { for (size_t i = ib; i < ie; i++) { const size_t j = L - 1 - i; const char a = s[i], c = s[j]; s[i] = rev_map(c); s[j] = rev_map(a); } };
	if (big) {
		par_ranges(fillable, (size_t)1 << 18, fill);
		if (L > fillable) { memset(t1.p + fillable, 0, L - fillable); memset(t2.p + fillable, 0, L - fillable); }      // (std::string::resize pads with NULs)
		par_ranges(L, (size_t)1 << 18, gaps);
		if (!b.bdir) {
			par_ranges(L / 2, (size_t)1 << 18, [&](size_t ib, size_t ie) { revpair(t1.p, ib, ie); revpair(t2.p, ib, ie); });
			if (L & 1) { t1.p[L / 2] = rev_map(t1.p[L / 2]); t2.p[L / 2] = rev_map(t2.p[L / 2]); }
		}
	} else {
		if (fillable) fill(0, fillable);
		if (L > fillable) { memset(t1.p + fillable, 0, L - fillable); memset(t2.p + fillable, 0, L - fillable); }
		gaps(0, L);
		if (!b.bdir) { revpair(t1.p, 0, L / 2); revpair(t2.p, 0, L / 2); if (L & 1) { t1.p[L / 2] = rev_map(t1.p[L / 2]); t2.p[L / 2] = rev_map(t2.p[L / 2]); } }
	}
	// "%s": the line ends at the first NUL
	const size_t n1 = (size_t)((const char *)memchr(t1.p, 0, L) ? (const char *)memchr(t1.p, 0, L) - t1.p : (ptrdiff_t)L);
	const size_t n2 = (size_t)((const char *)memchr(t2.p, 0, L) ? (const char *)memchr(t2.p, 0, L) - t2.p : (ptrdiff_t)L);
	const std::string &rname = idx->chr_name[b.chr];
	std::string qname = q.name;
	if (qname.size() <= rname.size()) qname.append(rname.size() - qname.size(), ' ');           // only the query name is printed padded (App. B #18)
	const int clen = idx->chr_len[b.chr]; const unsigned qlen = (unsigned)q.seq.size();
	std::vector<char> h1(rname.size() + 128), h2(qname.size() + 128);
	int l1, l2;
	if (b.bdir) {
		l1 = snprintf(h1.data(), h1.size(), "a score=%d\ns ref.%s %d %d + %d ", b.bdup ? 1 : b.score, rname.c_str(), b.gpos - 1, b.aln_len - (int)g1.load(), clen);
		l2 = snprintf(h2.data(), h2.size(), "\ns qry.%s %d %d + %d ", qname.c_str(), r.frag(f0).qpos, b.aln_len - (int)g2.load(), qlen);
	} else {
		const int64_t rpos = last.rpos + last.rlen - 1;
		int d, c, g; idx->coordinate(rpos, &d, &c, &g);
		l1 = snprintf(h1.data(), h1.size(), "a score=%d\ns ref.%s %d %d + %d ", b.bdup ? 1 : b.score, rname.c_str(), g - 1, b.aln_len - (int)g1.load(), clen);
		l2 = snprintf(h2.data(), h2.size(), "\ns qry.%s %d %d - %d ", qname.c_str(), qlen - (last.qpos + last.qlen), b.aln_len - (int)g2.load(), qlen);
	}
	if (!big) {
		small.append(h1.data(), (size_t)l1); small.append(t1.p, n1); small.append(h2.data(), (size_t)l2); small.append(t2.p, n2); small.append("\n\n", 2);
		if (small.n >= ((size_t)4 << 20)) { OutBuf out = std::move(small); small = OutBuf(); sink(std::move(out)); }
		return;
	}
	small.append(h1.data(), (size_t)l1);
	{ OutBuf out = std::move(small); small = OutBuf(); sink(std::move(out)); }
	t1.n = n1; sink(std::move(t1));
	small.append(h2.data(), (size_t)l2);
	{ OutBuf out = std::move(small); small = OutBuf(); sink(std::move(out)); }
	t2.n = n2; sink(std::move(t2));
	small.append("\n\n", 2);
}

void Emitter::maf_text(bool first, const QueryContig &q, ContigResult &r, const std::function<void(OutBuf &&)> &sink, const std::function<OutBuf(size_t)> &take) const
{
	OutBuf small;
	if (first) small.append("##maf version=1\n", 16);
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		gsa_block &b = r.blocks[bi];
		if (!allow_dup && b.bdup) continue;
		maf_block(q, r, b, small, sink, take);
	}
	if (small.n) sink(std::move(small));
}

void Emitter::maf(FILE *fp, bool first, const QueryContig &q, ContigResult &r) const
{
	maf_text(first, q, r, [&](OutBuf &&o) { if (o.n) fwrite(o.p, 1, o.n, fp); }, [](size_t c) { return OutBuf(c); });
}

// ---- PAF ------------------------------------------------------------------------------------------------------------------------------
namespace {
inline char *put_int(char *p, long long v)
{
	char tmp[24]; int n = 0; bool neg = v < 0; unsigned long long u = neg ? 0ull - (unsigned long long)v : (unsigned long long)v;
	do { tmp[n++] = (char)('0' + u % 10); u /= 10; } while (u);
	if (neg) *p++ = '-';
	while (n) *p++ = tmp[--n];
	return p;
}

inline uint32_t column_class(char a1, char a2)      // gsa_hip.h: reference row, query row
{
	if (a1 == '-') return GSA_CIGAR_INS;
	if (a2 == '-') return GSA_CIGAR_DEL;
	const int x = nt4((unsigned char)a1);
	return x < 4 && x == nt4((unsigned char)a2) ? GSA_CIGAR_EQ : GSA_CIGAR_X;
}
inline int32_t *class_count(gsa_block_cigar &bc, uint32_t cls) { return cls == GSA_CIGAR_EQ ? &bc.n_eq : (cls == GSA_CIGAR_X ? &bc.n_x : (cls == GSA_CIGAR_INS ? &bc.n_ins : &bc.n_del)); }
}

void gsah_block_cigars(const char *seq, const ContigResult &r, std::vector<gsa_block_cigar> &blk, std::vector<uint32_t> &ops)
{
	blk.assign(r.blocks.size(), gsa_block_cigar());
	ops.clear();
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		const gsa_block &b = r.blocks[bi];
		gsa_block_cigar &bc = blk[bi];
		memset(&bc, 0, sizeof(bc));
		bc.cig_off = (int64_t)ops.size();
		uint32_t cur = 0; uint64_t run = 0;
		auto column = [&](uint32_t cls) {
			if (cls != cur) { if (run) ops.push_back((uint32_t)(run << 4) | cur); cur = cls; run = 0; }
			run++; (*class_count(bc, cls))++;
		};
		for (int64_t k = 0; k < b.n_frag; k++) {
			const gsa_frag f = r.frag(b.frag_off + k);
			if (f.bseed) { for (int i = 0; i < f.qlen; i++) column(seq ? column_class(seq[f.qpos + i], seq[f.qpos + i]) : GSA_CIGAR_EQ); }      // a seed prints the QUERY text on both lines
			else { const char *x1 = r.aln1.data() + f.aln_off, *x2 = r.aln2.data() + f.aln_off; for (int i = 0; i < f.aln_len; i++) column(column_class(x1[i], x2[i])); }
		}
		if (run) ops.push_back((uint32_t)(run << 4) | cur);
		bc.n_cig = (int32_t)((int64_t)ops.size() - bc.cig_off);
		if (!b.bdir) std::reverse(ops.begin() + bc.cig_off, ops.end());      // SelfComplementarySeq: the two lines are printed back to front
	}
}

void gsah_cigar_trim(const uint32_t *ops, int bdir, int64_t ext, std::vector<uint32_t> &out, gsa_block_cigar &bc)
{
	int64_t lo = 0, hi = bc.n_cig;      // the ops that stay: [lo, hi), the one at the cut shortened
	uint32_t edge = 0; bool cut = false;
	while (ext > 0 && lo < hi) {
		const int64_t at = bdir ? hi - 1 : lo;
		const uint32_t cls = ops[at] & 15u; const int64_t len = ops[at] >> 4;
		const int64_t take = len <= ext ? len : ext;
		*class_count(bc, cls) -= (int32_t)take; ext -= take;
		if (take == len) { if (bdir) hi--; else lo++; }
		else { edge = (uint32_t)((len - take) << 4) | cls; cut = true; }
	}
	out.assign(ops + lo, ops + hi);
	if (cut && !out.empty()) { if (bdir) out.back() = edge; else out.front() = edge; }
	bc.n_cig = (int32_t)out.size();
}

namespace {
inline char cs_letter(char b, bool fwd) { return (fwd ? "acgtn" : "tgcan")[nt4((unsigned char)b)]; }
inline void cs_number(std::string &out, uint64_t v) { char tmp[24]; int n = 0; do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v); while (n) out.push_back(tmp[--n]); }
inline int64_t cs_op_bytes(uint32_t op)
{
	const uint32_t len = op >> 4, cls = op & 15u;
	if (cls != GSA_CIGAR_EQ) return cls == GSA_CIGAR_X ? 3 * (int64_t)len : 1 + (int64_t)len;
	int64_t n = 2; for (uint32_t v = len; v >= 10; v /= 10) n++;
	return n;
}
}

void gsah_block_cs(const ContigResult &r, std::vector<gsa_cs_block> &blk, std::string &cs)
{
	blk.assign(r.blocks.size(), gsa_cs_block());
	cs.clear();
	std::vector<uint8_t> cls; std::string t1, t2;      // the block's columns in walk order: class, reference row, query row (a seed's rows are not looked at)
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		const gsa_block &b = r.blocks[bi];
		cls.clear(); t1.clear(); t2.clear();
		for (int64_t k = 0; k < b.n_frag; k++) {
			const gsa_frag f = r.frag(b.frag_off + k);
			if (f.bseed) { if (f.qlen > 0) { cls.insert(cls.end(), (size_t)f.qlen, (uint8_t)GSA_CIGAR_EQ); t1.append((size_t)f.qlen, 'A'); t2.append((size_t)f.qlen, 'A'); } }
			else {
				const char *x1 = r.aln1.data() + f.aln_off, *x2 = r.aln2.data() + f.aln_off;
				for (int i = 0; i < f.aln_len; i++) cls.push_back((uint8_t)column_class(x1[i], x2[i]));
				if (f.aln_len > 0) { t1.append(x1, (size_t)f.aln_len); t2.append(x2, (size_t)f.aln_len); }
			}
		}
		const bool fwd = b.bdir != 0;
		if (!fwd) { std::reverse(cls.begin(), cls.end()); std::reverse(t1.begin(), t1.end()); std::reverse(t2.begin(), t2.end()); }      // SelfComplementarySeq
		const size_t at = cs.size();
		for (size_t i = 0; i < cls.size();) {
			size_t j = i; while (j < cls.size() && cls[j] == cls[i]) j++;
			if (cls[i] == GSA_CIGAR_EQ) { cs.push_back(':'); cs_number(cs, j - i); }
			else if (cls[i] == GSA_CIGAR_X) { for (size_t k = i; k < j; k++) { cs.push_back('*'); cs.push_back(cs_letter(t1[k], fwd)); cs.push_back(cs_letter(t2[k], fwd)); } }
			else if (cls[i] == GSA_CIGAR_INS) { cs.push_back('+'); for (size_t k = i; k < j; k++) cs.push_back(cs_letter(t2[k], fwd)); }
			else { cs.push_back('-'); for (size_t k = i; k < j; k++) cs.push_back(cs_letter(t1[k], fwd)); }
			i = j;
		}
		blk[bi].cs_off = (int64_t)at; blk[bi].n_cs = (int32_t)(cs.size() - at); blk[bi]._pad = 0;
	}
}

void gsah_cs_trim(const char *cs, int64_t n, const uint32_t *ops, int64_t n_ops, int bdir, int64_t ext, std::string &out)
{
	out.clear();
	int64_t lo = 0, hi = n_ops, b0 = 0, b1 = n;      // the ops that stay whole: [lo, hi), their bytes: [b0, b1)
	std::string edge;                                // what is left of the op at the cut
	while (ext > 0 && lo < hi) {
		const int64_t at = bdir ? hi - 1 : lo;
		const uint32_t cls = ops[at] & 15u; const int64_t len = ops[at] >> 4, bytes = cs_op_bytes(ops[at]);
		const int64_t take = len <= ext ? len : ext;
		ext -= take;
		const int64_t p = bdir ? b1 - bytes : b0;    // the op's first byte
		if (bdir) { hi--; b1 -= bytes; } else { lo++; b0 += bytes; }
		if (take == len) continue;
		const int64_t keep = len - take;
		if (p < 0 || p + bytes > n) break;           // (a string that is not the ops': nothing is read outside it)
		if (cls == GSA_CIGAR_EQ) { edge.push_back(':'); cs_number(edge, (uint64_t)keep); }
		else if (cls == GSA_CIGAR_X) edge.assign(cs + p + (bdir ? 0 : 3 * take), (size_t)(3 * keep));
		else { edge.push_back(cs[p]); edge.append(cs + p + 1 + (bdir ? 0 : take), (size_t)keep); }
	}
	if (b1 > n) b1 = n;
	if (!bdir) out += edge;
	if (b1 > b0) out.append(cs + b0, (size_t)(b1 - b0));
	if (bdir) out += edge;
}

void Emitter::paf_text(const QueryContig &q, ContigResult &r, const gsa_block_cigar *blk, const uint32_t *ops, const std::function<void(OutBuf &&)> &sink,
                       const gsa_cs_block *csb, const char *cs) const
{
	std::vector<gsa_block_cigar> own_blk; std::vector<uint32_t> own_ops, cut; std::string cs_cut;
	if (!blk && r.summary) return;      // (the comparator walks records and strings a summary result does not hold)
	if (!blk) { gsah_block_cigars(q.seq.data(), r, own_blk, own_ops); blk = own_blk.data(); ops = own_ops.data(); }
	OutBuf o;
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		gsa_block &b = r.blocks[bi];
		if (!allow_dup && b.bdup) continue;
		if (b.n_frag <= 0) continue;
		// the block's first and last record: where frag_off / n_frag say, or -- summary mode -- the block's two ends
		const int64_t f0 = r.summary ? 2 * (int64_t)bi : b.frag_off, fl = r.summary ? 2 * (int64_t)bi + 1 : b.frag_off + b.n_frag - 1;
		gsa_frag last = r.frag(fl);
		const int ext = extension(*idx, b, last);
		gsa_block_cigar bc = blk[bi];
		const uint32_t *bo = ops + bc.cig_off;
		const char *bcs = csb ? cs + csb[bi].cs_off : nullptr; size_t n_bcs = csb ? (size_t)csb[bi].n_cs : 0;
		if (csb && ext > 0) { gsah_cs_trim(bcs, (int64_t)n_bcs, bo, bc.n_cig, b.bdir, ext, cs_cut); bcs = cs_cut.data(); n_bcs = cs_cut.size(); }      // (from the untrimmed ops)
		if (ext > 0) {      // (as maf_block: the block and its last record are shortened for whoever looks at them next -- the variant walk, the dot plot)
			b.aln_len -= ext; b.score -= ext; last.rlen -= ext; last.qlen -= ext; r.trim(fl, ext);
			gsah_cigar_trim(bo, b.bdir, ext, cut, bc); bo = cut.data();
		}
		const long long cols = (long long)bc.n_eq + bc.n_x + bc.n_ins + bc.n_del;
		const long long qbases = (long long)bc.n_eq + bc.n_x + bc.n_ins, rbases = (long long)bc.n_eq + bc.n_x + bc.n_del;
		const long long qsize = (long long)q.seq.size();
		long long qs, qe, ts;
		if (b.bdir) { qs = r.frag(f0).qpos; qe = qs + qbases; ts = b.gpos - 1; }
		else {
			// the MAF line gives start = qlen - (last.qpos + last.qlen) on the '-' strand: on the forward strand the block ends there
			qe = (long long)last.qpos + last.qlen; qs = qe - qbases;
			int d, c, g; idx->coordinate(last.rpos + last.rlen - 1, &d, &c, &g); ts = g - 1;
		}
		const std::string &rname = idx->chr_name[b.chr];
		o.reserve(o.n + q.name.size() + rname.size() + 256 + (size_t)bc.n_cig * 11 + n_bcs);
		char *w = o.p + o.n;
		memcpy(w, q.name.data(), q.name.size()); w += q.name.size(); *w++ = '\t';
		w = put_int(w, qsize); *w++ = '\t'; w = put_int(w, qs); *w++ = '\t'; w = put_int(w, qe); *w++ = '\t';
		*w++ = b.bdir ? '+' : '-'; *w++ = '\t';
		memcpy(w, rname.data(), rname.size()); w += rname.size(); *w++ = '\t';
		w = put_int(w, idx->chr_len[b.chr]); *w++ = '\t'; w = put_int(w, ts); *w++ = '\t'; w = put_int(w, ts + rbases); *w++ = '\t';
		w = put_int(w, bc.n_eq); *w++ = '\t'; w = put_int(w, cols); memcpy(w, "\t255\tNM:i:", 10); w += 10;
		w = put_int(w, (long long)bc.n_x + bc.n_ins + bc.n_del); memcpy(w, "\tAS:i:", 6); w += 6;
		w = put_int(w, b.bdup ? 1 : b.score); memcpy(w, b.bdup ? "\ttp:A:S\tcg:Z:" : "\ttp:A:P\tcg:Z:", 13); w += 13;
		w += gsa_cigar_string(bo, bc.n_cig, w, (size_t)bc.n_cig * 11 + 1);
		if (csb) { memcpy(w, "\tcs:Z:", 6); w += 6; if (n_bcs) memcpy(w, bcs, n_bcs); w += n_bcs; }
		*w++ = '\n';
		o.n = (size_t)(w - o.p);
		if (o.n >= ((size_t)4 << 20)) { OutBuf out = std::move(o); o = OutBuf(); sink(std::move(out)); }
	}
	if (o.n) sink(std::move(o));
}

void Emitter::paf(FILE *fp, const QueryContig &q, ContigResult &r, const gsa_block_cigar *blk, const uint32_t *ops, const gsa_cs_block *csb, const char *cs) const
{
	paf_text(q, r, blk, ops, [&](OutBuf &&o) { if (o.n) fwrite(o.p, 1, o.n, fp); }, csb, cs);
}

// ---- chain segments -----------------------------------------------------------------------------------------------------------------------
void gsah_block_segs(const ContigResult &r, std::vector<gsa_seg_block> &blk, std::vector<gsa_seg> &segs)
{
	blk.assign(r.blocks.size(), gsa_seg_block());
	segs.clear();
	std::vector<gsa_seg> w;                       // the block's triples in walk order: {size, gap behind it}
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		const gsa_block &b = r.blocks[bi];
		w.clear();
		bool in_seg = false; int32_t dt = 0, dq = 0;      // the gap columns seen since the last aligned one
		auto aligned = [&](int64_t n) {
			if (n <= 0) return;
			if (!in_seg) { if (!w.empty()) { w.back().dt = dt; w.back().dq = dq; } const gsa_seg s = { 0, 0, 0 }; w.push_back(s); in_seg = true; }
			w.back().size += (int32_t)n;
		};
		auto gap = [&](bool ref_base) { if (in_seg) { in_seg = false; dt = dq = 0; } if (ref_base) dt++; else dq++; };      // (in front of the first segment: counted and never stored)
		for (int64_t k = 0; k < b.n_frag; k++) {
			const gsa_frag f = r.frag(b.frag_off + k);
			if (f.bseed) aligned(f.qlen);
			else {
				const char *x1 = r.aln1.data() + f.aln_off, *x2 = r.aln2.data() + f.aln_off;
				for (int i = 0; i < f.aln_len; i++) { if (x1[i] == '-') gap(false); else if (x2[i] == '-') gap(true); else aligned(1); }
			}
		}
		blk[bi].seg_off = (int64_t)segs.size(); blk[bi].n_seg = (int32_t)w.size(); blk[bi]._pad = 0;
		if (b.bdir) segs.insert(segs.end(), w.begin(), w.end());
		else for (size_t k = w.size(); k-- > 0;) { gsa_seg s = { w[k].size, 0, 0 }; if (k > 0) { s.dt = w[k - 1].dt; s.dq = w[k - 1].dq; } segs.push_back(s); }      // SelfComplementarySeq: back to front, the gap in front comes behind
	}
}

void gsah_segs_trim(const gsa_seg *segs, int64_t n, int bdir, int64_t ext, std::vector<gsa_seg> &out)
{
	int64_t lo = 0, hi = n, edge = -1;      // the triples that stay: [lo, hi); edge: what is left of the segment at the cut
	while (ext > 0 && lo < hi) {
		const gsa_seg &s = segs[bdir ? hi - 1 : lo];
		if (ext < s.size) { edge = s.size - ext; ext = 0; break; }
		ext -= s.size;
		if (bdir) hi--; else lo++;
		if (lo >= hi) break;
		// the gap that is now at the end, in walk order in front of the segment that went: a forward block's lies in the triple in front, a reverse-strand block's in the triple that went
		const gsa_seg &g = bdir ? segs[hi - 1] : s;
		const int64_t cols = (int64_t)g.dt + g.dq;
		ext -= ext < cols ? ext : cols;
	}
	out.assign(segs + lo, segs + hi);
	if (!out.empty()) {
		if (edge >= 0) { if (bdir) out.back().size = (int32_t)edge; else out.front().size = (int32_t)edge; }
		out.back().dt = 0; out.back().dq = 0;
	}
}

// ---- lifted reference positions ----------------------------------------------------------------------------------------------------------
void gsah_lift(const HostIndex &ix, const ContigResult &r, const int64_t *pos, int64_t n, std::vector<gsa_lift_hit> &hits)
{
	hits.clear();
	if (r.summary || n <= 0) return;      // (a summary result holds neither records nor strings)
	// the blocks with records in the order of their first text position, the running maximum of their trimmed ends beside them
	struct Blk { int64_t start, end, maxend; int32_t block; };
	std::vector<Blk> tab;
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		const gsa_block &b = r.blocks[bi];
		if (b.n_frag <= 0) continue;
		const gsa_frag first = r.frag(b.frag_off), last = r.frag(b.frag_off + b.n_frag - 1);
		Blk v; v.start = first.rpos; v.end = last.rpos + last.rlen - extension(ix, b, last); v.maxend = 0; v.block = (int32_t)bi;
		if (v.end > v.start) tab.push_back(v);
	}
	if (tab.empty()) return;
	std::sort(tab.begin(), tab.end(), [](const Blk &x, const Blk &y) { return x.start != y.start ? x.start < y.start : x.block < y.block; });
	for (size_t j = 0; j < tab.size(); j++) tab[j].maxend = j ? std::max(tab[j - 1].maxend, tab[j].end) : tab[j].end;
	auto better = [&](int32_t x, int32_t y) {
		const gsa_block &a = r.blocks[(size_t)x], &b = r.blocks[(size_t)y];
		if ((a.bdup != 0) != (b.bdup != 0)) return a.bdup == 0;
		if (a.score != b.score) return a.score > b.score;
		return x < y;
	};
	auto cover = [&](int64_t t, int32_t &best, uint32_t &cnt) {
		size_t j = (size_t)(std::upper_bound(tab.begin(), tab.end(), t, [](int64_t v, const Blk &b) { return v < b.start; }) - tab.begin());
		while (j > 0 && tab[j - 1].maxend > t) {
			j--;
			if (tab[j].end <= t) continue;
			cnt++;
			if (best < 0 || better(tab[j].block, best)) best = tab[j].block;
		}
	};
	std::vector<gsa_lift_hit> all((size_t)n);      // cls = 0: no block covers the position
	auto one = [&](size_t ib, size_t ie) {
		for (size_t i = ib; i < ie; i++) {
			gsa_lift_hit &h = all[i];
			memset(&h, 0, sizeof(h));
			const int64_t p = pos[i];
			if (p < 0 || p >= ix.G) continue;
			int32_t best = -1; uint32_t cnt = 0;
			cover(p, best, cnt); cover(2 * ix.G - 1 - p, best, cnt);
			if (best < 0) continue;
			const gsa_block &b = r.blocks[(size_t)best];
			const int64_t t = b.bdir ? p : 2 * ix.G - 1 - p;
			int64_t lo = b.frag_off, hi = b.frag_off + b.n_frag;      // the last record that starts at or before t
			while (hi - lo > 1) { const int64_t m = (lo + hi) >> 1; if (r.frag(m).rpos <= t) lo = m; else hi = m; }
			const gsa_frag f = r.frag(lo);
			const int64_t d = t - f.rpos;
			h.idx = (int32_t)i; h.block = best; h.rev = b.bdir ? 0 : 1; h.n_cover = (uint16_t)(cnt > 65535u ? 65535u : cnt);
			if (f.bseed) { h.cls = (uint8_t)GSA_CIGAR_EQ; h.qpos = f.qpos + (int32_t)d; continue; }
			const char *x1 = r.aln1.data() + f.aln_off, *x2 = r.aln2.data() + f.aln_off;
			int64_t rp = f.rpos; int32_t qp = f.qpos;
			h.qpos = -1;
			for (int c = 0; c < f.aln_len; c++) {
				if (x1[c] != '-' && rp == t) {
					if (x2[c] == '-') { h.cls = (uint8_t)GSA_CIGAR_DEL; h.qpos = qp - 1; }
					else { h.cls = (uint8_t)column_class(x1[c], x2[c]); h.qpos = qp; }
					break;
				}
				if (x1[c] != '-') rp++;
				if (x2[c] != '-') qp++;
			}
		}
	};
	if ((size_t)n * sizeof(gsa_lift_hit) >= par_min_bytes()) par_ranges((size_t)n, (size_t)1 << 14, one); else one(0, (size_t)n);
	for (size_t i = 0; i < (size_t)n; i++) if (all[i].cls) hits.push_back(all[i]);
}

// <prefix>.lift.tsv: one line per hit -- reference name, 1-based position, query name, 1-based query position, strand, class letter, the block's score as the MAF
// prints it (trimmed; 1 for a duplicate), n_cover.  ref_chr / ref_pos: sequence and 1-based position of every input position (hit::idx indexes them)
void Emitter::lift_text(bool first, const QueryContig &q, const ContigResult &r, const gsa_lift_hit *hits, int64_t n_hits, const int32_t *ref_chr, const int32_t *ref_pos,
                        const std::function<void(OutBuf &&)> &sink) const
{
	OutBuf o;
	if (first) o.append("#ref\tpos\tquery\tqpos\tstrand\tclass\tscore\tn_cover\n");
	std::vector<int> score(r.blocks.size(), 0);
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		const gsa_block &b = r.blocks[bi];
		score[bi] = b.bdup ? 1 : b.score;
		if (!b.bdup && b.n_frag > 0 && !r.summary) score[bi] -= extension(*idx, b, r.frag(b.frag_off + b.n_frag - 1));
	}
	for (int64_t i = 0; i < n_hits; i++) {
		const gsa_lift_hit &h = hits[i];
		if (h.block < 0 || (size_t)h.block >= r.blocks.size()) continue;
		const std::string &rname = idx->chr_name[(size_t)ref_chr[h.idx]];
		o.reserve(o.n + rname.size() + q.name.size() + 96);
		char *w = o.p + o.n;
		memcpy(w, rname.data(), rname.size()); w += rname.size(); *w++ = '\t';
		w = put_int(w, ref_pos[h.idx]); *w++ = '\t';
		memcpy(w, q.name.data(), q.name.size()); w += q.name.size(); *w++ = '\t';
		w = put_int(w, (long long)h.qpos + 1); *w++ = '\t';
		*w++ = h.rev ? '-' : '+'; *w++ = '\t';
		*w++ = h.cls == GSA_CIGAR_EQ ? '=' : (h.cls == GSA_CIGAR_X ? 'X' : 'D'); *w++ = '\t';
		w = put_int(w, score[(size_t)h.block]); *w++ = '\t';
		w = put_int(w, h.n_cover); *w++ = '\n';
		o.n = (size_t)(w - o.p);
		if (o.n >= ((size_t)4 << 20)) { OutBuf out = std::move(o); o = OutBuf(); sink(std::move(out)); }
	}
	if (o.n) sink(std::move(o));
}

// ---- lifted reference intervals ----------------------------------------------------------------------------------------------------------
void gsah_lift_regions(const HostIndex &ix, const ContigResult &r, const int64_t *beg, const int64_t *end, int64_t n, std::vector<gsa_region_hit> &hits)
{
	hits.clear();
	if (r.summary || n <= 0) return;      // (a summary result holds neither records nor strings)
	// the blocks with records in the order of their first text position, the running maximum of their trimmed ends beside them (as gsah_lift)
	struct Blk { int64_t start, end, maxend; int32_t block; };
	std::vector<Blk> tab;
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		const gsa_block &b = r.blocks[bi];
		if (b.n_frag <= 0) continue;
		const gsa_frag first = r.frag(b.frag_off), last = r.frag(b.frag_off + b.n_frag - 1);
		Blk v; v.start = first.rpos; v.end = last.rpos + last.rlen - extension(ix, b, last); v.maxend = 0; v.block = (int32_t)bi;
		if (v.end > v.start) tab.push_back(v);
	}
	if (tab.empty()) return;
	std::sort(tab.begin(), tab.end(), [](const Blk &x, const Blk &y) { return x.start != y.start ? x.start < y.start : x.block < y.block; });
	for (size_t j = 0; j < tab.size(); j++) tab[j].maxend = j ? std::max(tab[j - 1].maxend, tab[j].end) : tab[j].end;
	struct Best { int32_t block = -1; int64_t ov = 0, start = 0, end = 0; };
	auto better = [&](int32_t x, int64_t ox, const Best &y) {
		const gsa_block &a = r.blocks[(size_t)x], &b = r.blocks[(size_t)y.block];
		if ((a.bdup != 0) != (b.bdup != 0)) return a.bdup == 0;
		if (ox != y.ov) return ox > y.ov;
		if (a.score != b.score) return a.score > b.score;
		return x < y.block;
	};
	auto cover = [&](int64_t lo, int64_t hi, Best &best, uint32_t &cnt) {      // the blocks whose coverage overlaps the text interval [lo, hi)
		size_t j = (size_t)(std::lower_bound(tab.begin(), tab.end(), hi, [](const Blk &b, int64_t v) { return b.start < v; }) - tab.begin());
		while (j > 0 && tab[j - 1].maxend > lo) {
			j--;
			if (tab[j].end <= lo) continue;
			const int64_t ov = std::min(tab[j].end, hi) - std::max(tab[j].start, lo);
			cnt++;
			if (best.block < 0 || better(tab[j].block, ov, best)) { best.block = tab[j].block; best.ov = ov; best.start = tab[j].start; best.end = tab[j].end; }
		}
	};
	std::vector<gsa_region_hit> all((size_t)n);      // block = -1: no block overlaps the region
	auto one = [&](size_t ib, size_t ie) {
		for (size_t i = ib; i < ie; i++) {
			gsa_region_hit &h = all[i];
			memset(&h, 0, sizeof(h)); h.block = -1;
			const int64_t p0 = beg[i], p1 = end[i];
			if (p0 < 0 || p0 >= p1 || p1 > ix.G) continue;
			{      // (a region that crosses a sequence boundary is no region: gsa_regions_set refuses it)
				size_t c = 0; while (c + 1 < ix.chr_fwd.size() && ix.chr_fwd[c + 1] <= p0) c++;
				if (p1 > ix.chr_fwd[c] + ix.chr_len[c]) continue;
			}
			Best best; uint32_t cnt = 0;
			cover(p0, p1, best, cnt); cover(2 * ix.G - p1, 2 * ix.G - p0, best, cnt);
			if (best.block < 0) continue;
			const gsa_block &b = r.blocks[(size_t)best.block];
			const int64_t lo = b.bdir ? p0 : 2 * ix.G - p1, hi = b.bdir ? p1 : 2 * ix.G - p0;
			const int64_t t_lo = std::max(lo, best.start), t_hi = std::min(hi, best.end);
			h.idx = (int32_t)i; h.block = best.block; h.rev = b.bdir ? 0 : 1; h.n_cover = (uint16_t)(cnt > 65535u ? 65535u : cnt);
			h.off_lo = (int32_t)(b.bdir ? t_lo - lo : hi - t_hi); h.off_hi = (int32_t)(b.bdir ? t_hi - lo : hi - t_lo);
			int64_t a = b.frag_off, z = b.frag_off + b.n_frag;      // the last record that starts at or before t_lo
			while (z - a > 1) { const int64_t m = (a + z) >> 1; if (r.frag(m).rpos <= t_lo) a = m; else z = m; }
			// the columns in walk order from the one that holds t_lo through the one that holds t_hi - 1
			bool in = false, done = false; int32_t q_lo = -1;
			for (int64_t k = a; k < b.frag_off + b.n_frag && !done; k++) {
				const gsa_frag f = r.frag(k);
				if (f.bseed) {
					const int64_t s = std::max<int64_t>(f.rpos, t_lo), e = std::min<int64_t>(f.rpos + f.rlen, t_hi);
					if (e <= s) continue;
					if (!in) { in = true; q_lo = f.qpos + (int32_t)(s - f.rpos); }
					h.n_eq += (uint32_t)(e - s);
					if (e == t_hi) done = true;
					continue;
				}
				const char *x1 = r.aln1.data() + f.aln_off, *x2 = r.aln2.data() + f.aln_off;
				int64_t rp = f.rpos; int32_t qp = f.qpos;
				for (int c = 0; c < f.aln_len; c++) {
					const bool rb = x1[c] != '-', qb = x2[c] != '-';
					if (!in && rb && rp == t_lo) { in = true; q_lo = qp; }
					if (in) {
						if (!rb) h.n_ins++;
						else if (!qb) h.n_del++;
						else if (column_class(x1[c], x2[c]) == (int)GSA_CIGAR_EQ) h.n_eq++;
						else h.n_x++;
						if (rb && rp == t_hi - 1) { done = true; break; }
					}
					if (rb) rp++;
					if (qb) qp++;
				}
			}
			h.q_lo = q_lo; h.q_hi = q_lo + (int32_t)(h.n_eq + h.n_x + h.n_ins);
		}
	};
	if ((size_t)n * sizeof(gsa_region_hit) >= par_min_bytes()) par_ranges((size_t)n, (size_t)1 << 12, one); else one(0, (size_t)n);
	for (size_t i = 0; i < (size_t)n; i++) if (all[i].block >= 0) hits.push_back(all[i]);
}

// <prefix>.regions.tsv: one line per hit -- reference name, the region (0-based, half-open, inside the sequence), its name, the covered part, query name, the query
// interval (0-based, half-open, in the contig as stored), strand, the four counts, the block's score as the MAF prints it (trimmed; 1 for a duplicate), n_cover
void Emitter::regions_text(bool first, const QueryContig &q, const ContigResult &r, const gsa_region_hit *hits, int64_t n_hits, const int32_t *ref_chr, const int32_t *ref_beg,
                           const int32_t *ref_end, const std::string *name, const std::function<void(OutBuf &&)> &sink) const
{
	OutBuf o;
	if (first) o.append("#ref\tstart\tend\tname\tcstart\tcend\tquery\tqstart\tqend\tstrand\tmatch\tmismatch\tdeleted\tinserted\tscore\tn_cover\n");
	std::vector<int> score(r.blocks.size(), 0);
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		const gsa_block &b = r.blocks[bi];
		score[bi] = b.bdup ? 1 : b.score;
		if (!b.bdup && b.n_frag > 0 && !r.summary) score[bi] -= extension(*idx, b, r.frag(b.frag_off + b.n_frag - 1));
	}
	for (int64_t i = 0; i < n_hits; i++) {
		const gsa_region_hit &h = hits[i];
		if (h.block < 0 || (size_t)h.block >= r.blocks.size()) continue;
		const std::string &rname = idx->chr_name[(size_t)ref_chr[h.idx]], &nm = name[h.idx];
		o.reserve(o.n + rname.size() + nm.size() + q.name.size() + 256);
		char *w = o.p + o.n;
		memcpy(w, rname.data(), rname.size()); w += rname.size(); *w++ = '\t';
		w = put_int(w, ref_beg[h.idx]); *w++ = '\t'; w = put_int(w, ref_end[h.idx]); *w++ = '\t';
		memcpy(w, nm.data(), nm.size()); w += nm.size(); *w++ = '\t';
		w = put_int(w, (long long)ref_beg[h.idx] + h.off_lo); *w++ = '\t'; w = put_int(w, (long long)ref_beg[h.idx] + h.off_hi); *w++ = '\t';
		memcpy(w, q.name.data(), q.name.size()); w += q.name.size(); *w++ = '\t';
		w = put_int(w, h.q_lo); *w++ = '\t'; w = put_int(w, h.q_hi); *w++ = '\t';
		*w++ = h.rev ? '-' : '+'; *w++ = '\t';
		w = put_int(w, h.n_eq); *w++ = '\t'; w = put_int(w, h.n_x); *w++ = '\t'; w = put_int(w, h.n_del); *w++ = '\t'; w = put_int(w, h.n_ins); *w++ = '\t';
		w = put_int(w, score[(size_t)h.block]); *w++ = '\t';
		w = put_int(w, h.n_cover); *w++ = '\n';
		o.n = (size_t)(w - o.p);
		if (o.n >= ((size_t)4 << 20)) { OutBuf out = std::move(o); o = OutBuf(); sink(std::move(out)); }
	}
	if (o.n) sink(std::move(o));
}

// ---- UCSC chain ----------------------------------------------------------------------------------------------------------------------------
void Emitter::chain_text(const QueryContig &q, const ContigResult &r, const gsa_seg_block *blk, const gsa_seg *seg, int64_t *id, const std::function<void(OutBuf &&)> &sink) const
{
	std::vector<gsa_seg_block> own_blk; std::vector<gsa_seg> own_seg, cut;
	if (r.summary) return;      // (a summary result holds no untrimmed last record per block in the place this walk looks, and the comparator needs the strings)
	if (!blk) { gsah_block_segs(r, own_blk, own_seg); blk = own_blk.data(); seg = own_seg.data(); }
	OutBuf o;
	const long long qsize = (long long)q.seq.size();
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		const gsa_block &b = r.blocks[bi];
		if (!allow_dup && b.bdup) continue;
		if (b.n_frag <= 0 || blk[bi].n_seg <= 0) continue;
		const gsa_frag first = r.frag(b.frag_off), last = r.frag(b.frag_off + b.n_frag - 1);
		const int ext = extension(*idx, b, last);
		const gsa_seg *bs = seg + blk[bi].seg_off; int64_t ns = blk[bi].n_seg;
		if (ext > 0) { gsah_segs_trim(bs, ns, b.bdir, ext, cut); bs = cut.data(); ns = (int64_t)cut.size(); }
		if (ns <= 0) continue;
		long long tbases = 0, qbases = 0;
		for (int64_t k = 0; k < ns; k++) { tbases += (long long)bs[k].size + bs[k].dt; qbases += (long long)bs[k].size + bs[k].dq; }
		long long ts, qs;
		if (b.bdir) { ts = b.gpos - 1; qs = first.qpos; }
		else {
			// the block ends, in walk order, where it starts in the output.  The MAF line starts at the end of the last record shortened by ext (tools.cpp:192-202, every cut
			// column taken as a base of either side); gap columns the cut left at that edge go with their gap, and their bases move the start on
			long long rem_d = 0, rem_i = 0;
			if (ext > 0) {
				int64_t skip = ext; bool done = false;
				for (int64_t k = b.n_frag - 1; k >= 0 && !done; k--) {
					const gsa_frag f = r.frag(b.frag_off + k);
					const int64_t L = f.bseed ? f.qlen : f.aln_len;
					if (L <= 0) continue;
					if (skip >= L) { skip -= L; continue; }
					if (f.bseed) break;
					const char *x1 = r.aln1.data() + f.aln_off, *x2 = r.aln2.data() + f.aln_off;
					for (int64_t i = L - 1 - skip; i >= 0; i--) { if (x1[i] == '-') rem_i++; else if (x2[i] == '-') rem_d++; else { done = true; break; } }
					skip = 0;
				}
			}
			int d, c, g; idx->coordinate(last.rpos + last.rlen - ext - rem_d - 1, &d, &c, &g); ts = g - 1;
			qs = qsize - ((long long)last.qpos + last.qlen - ext - rem_i);
		}
		const std::string &rname = idx->chr_name[b.chr];
		o.reserve(o.n + q.name.size() + rname.size() + 256 + (size_t)ns * 36);
		char *w = o.p + o.n;
		memcpy(w, "chain ", 6); w += 6; w = put_int(w, b.bdup ? 1 : b.score - ext); *w++ = ' ';
		memcpy(w, rname.data(), rname.size()); w += rname.size(); *w++ = ' ';
		w = put_int(w, idx->chr_len[b.chr]); memcpy(w, " + ", 3); w += 3; w = put_int(w, ts); *w++ = ' '; w = put_int(w, ts + tbases); *w++ = ' ';
		memcpy(w, q.name.data(), q.name.size()); w += q.name.size(); *w++ = ' ';
		w = put_int(w, qsize); *w++ = ' '; *w++ = b.bdir ? '+' : '-'; *w++ = ' '; w = put_int(w, qs); *w++ = ' '; w = put_int(w, qs + qbases); *w++ = ' ';
		w = put_int(w, ++*id); *w++ = '\n';
		for (int64_t k = 0; k + 1 < ns; k++) { w = put_int(w, bs[k].size); *w++ = '\t'; w = put_int(w, bs[k].dt); *w++ = '\t'; w = put_int(w, bs[k].dq); *w++ = '\n'; }
		w = put_int(w, bs[ns - 1].size); *w++ = '\n'; *w++ = '\n';
		o.n = (size_t)(w - o.p);
		if (o.n >= ((size_t)4 << 20)) { OutBuf out = std::move(o); o = OutBuf(); sink(std::move(out)); }
	}
	if (o.n) sink(std::move(o));
}

void Emitter::chain(FILE *fp, const QueryContig &q, const ContigResult &r, const gsa_seg_block *blk, const gsa_seg *seg, int64_t *id) const
{
	chain_text(q, r, blk, seg, id, [&](OutBuf &&o) { if (o.n) fwrite(o.p, 1, o.n, fp); });
}

// ---- per-window reference track ----------------------------------------------------------------------------------------------------------
void gsah_track(const HostIndex &ix, const ContigResult &r, int32_t W, std::vector<gsa_track_win> &win)
{
	win.clear();
	if (r.summary || W <= 0) return;      // (a summary result holds neither records nor strings)
	const size_t nchr = ix.chr_len.size();
	std::vector<int64_t> win0(nchr + 1, 0);      // first window of every sequence in the dense array
	for (size_t i = 0; i < nchr; i++) win0[i + 1] = win0[i] + ((int64_t)ix.chr_len[i] + W - 1) / W;
	struct Iv { int32_t chr; int64_t s, e; };
	std::vector<Iv> iv;                           // the counted blocks' trimmed spans in forward coordinates inside their sequence
	std::vector<uint32_t> bin;                    // {n_eq, n_x, n_del, n_ins} per window
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		const gsa_block &b = r.blocks[bi];
		if (b.bdup != 0 || b.n_frag <= 0 || b.chr < 0 || (size_t)b.chr >= nchr) continue;
		const gsa_frag first = r.frag(b.frag_off), last = r.frag(b.frag_off + b.n_frag - 1);
		const int64_t start = first.rpos, end = last.rpos + last.rlen - extension(ix, b, last);
		if (end <= start) continue;
		const bool rev = !b.bdir;
		const int64_t org = rev ? 2 * ix.G - 1 - ix.chr_fwd[b.chr] : ix.chr_fwd[b.chr], w0 = win0[(size_t)b.chr];
		Iv v; v.chr = b.chr; v.s = rev ? org - (end - 1) : start - org; v.e = rev ? org - start + 1 : end - org;
		iv.push_back(v);
		if (bin.empty()) bin.assign((size_t)win0[nchr] * 4, 0u);
		// a range of the block's records: the counts of one window are gathered while the walk stays in it and added when it leaves (several threads may meet in a window)
		auto piece = [&](size_t fb, size_t fe) {
			int64_t cur = -1; uint32_t cnt[4] = { 0, 0, 0, 0 };
			auto flush = [&] {
				if (cur >= 0) for (int f = 0; f < 4; f++) if (cnt[f]) __atomic_fetch_add(&bin[(size_t)cur * 4 + f], cnt[f], __ATOMIC_RELAXED);
				cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
			};
			// n columns of field f whose reference bases are the text positions t, t + 1, ...: split over the windows by arithmetic
			auto run = [&](int64_t t, int64_t n, int f) {
				if (t < start) { n -= start - t; t = start; }
				if (t + n > end) n = end - t;
				while (n > 0) {
					const int64_t l = rev ? org - t : t - org, j = l / W;
					const int64_t m = std::min<int64_t>(n, rev ? l - j * W + 1 : (j + 1) * W - l);
					if (w0 + j != cur) { flush(); cur = w0 + j; }
					cnt[f] += (uint32_t)m; t += m; n -= m;
				}
			};
			for (size_t k = fb; k < fe; k++) {
				const gsa_frag f = r.frag(b.frag_off + (int64_t)k);
				if (f.bseed) { run(f.rpos, f.rlen, 0); continue; }
				const char *x1 = r.aln1.data() + f.aln_off, *x2 = r.aln2.data() + f.aln_off;
				int64_t rp = f.rpos;
				for (int c = 0; c < f.aln_len; c++) {
					if (x1[c] == '-') { run(rp - 1, 1, 3); continue; }      // (an inserted query base belongs to the reference base consumed last)
					run(rp, 1, x2[c] == '-' ? 2 : (column_class(x1[c], x2[c]) == GSA_CIGAR_EQ ? 0 : 1));
					rp++;
				}
			}
			flush();
		};
		if ((size_t)b.n_frag * 16 >= par_min_bytes()) par_ranges((size_t)b.n_frag, (size_t)1 << 13, piece); else piece(0, (size_t)b.n_frag);
	}
	if (iv.empty()) return;
	std::sort(iv.begin(), iv.end(), [](const Iv &x, const Iv &y) { return x.chr != y.chr ? x.chr < y.chr : (x.s != y.s ? x.s < y.s : x.e < y.e); });
	size_t n = 0;
	for (size_t j = 0; j < iv.size(); j++) {
		if (n && iv[n - 1].chr == iv[j].chr && iv[j].s <= iv[n - 1].e) iv[n - 1].e = std::max(iv[n - 1].e, iv[j].e);
		else iv[n++] = iv[j];
	}
	// the windows the merged intervals touch, in order; n_cov: the union
	for (size_t m = 0; m < n; m++) {
		const int64_t len = ix.chr_len[(size_t)iv[m].chr];
		for (int64_t j = iv[m].s / W; j <= (iv[m].e - 1) / W; j++) {
			const int64_t lo = j * W, hi = std::min<int64_t>(lo + W, len);
			const uint32_t ov = (uint32_t)(std::min(iv[m].e, hi) - std::max(iv[m].s, lo));
			if (!win.empty() && win.back().chr == iv[m].chr && win.back().start == lo) { win.back().n_cov += ov; continue; }
			const uint32_t *c = &bin[(size_t)(win0[(size_t)iv[m].chr] + j) * 4];
			gsa_track_win w; w.chr = iv[m].chr; w.start = (int32_t)lo; w.len = (int32_t)(hi - lo); w.n_cov = ov; w.n_eq = c[0]; w.n_x = c[1]; w.n_del = c[2]; w.n_ins = c[3];
			win.push_back(w);
		}
	}
}

// <prefix>.track.tsv: one line per window -- reference name, BED-style start and end inside the sequence, query name, and the five counts
void Emitter::track_text(bool first, const QueryContig &q, const gsa_track_win *win, int64_t n_win, const std::function<void(OutBuf &&)> &sink) const
{
	OutBuf o;
	if (first) o.append("#ref\tstart\tend\tquery\tcovered\tmatch\tmismatch\tdeleted\tinserted\n");
	for (int64_t i = 0; i < n_win; i++) {
		const gsa_track_win &t = win[i];
		if (t.chr < 0 || (size_t)t.chr >= idx->chr_name.size()) continue;
		const std::string &rname = idx->chr_name[(size_t)t.chr];
		o.reserve(o.n + rname.size() + q.name.size() + 128);
		char *w = o.p + o.n;
		memcpy(w, rname.data(), rname.size()); w += rname.size(); *w++ = '\t';
		w = put_int(w, t.start); *w++ = '\t';
		w = put_int(w, (long long)t.start + t.len); *w++ = '\t';
		memcpy(w, q.name.data(), q.name.size()); w += q.name.size(); *w++ = '\t';
		w = put_int(w, (long long)t.n_cov); *w++ = '\t';
		w = put_int(w, (long long)t.n_eq); *w++ = '\t';
		w = put_int(w, (long long)t.n_x); *w++ = '\t';
		w = put_int(w, (long long)t.n_del); *w++ = '\t';
		w = put_int(w, (long long)t.n_ins); *w++ = '\n';
		o.n = (size_t)(w - o.p);
		if (o.n >= ((size_t)4 << 20)) { OutBuf out = std::move(o); o = OutBuf(); sink(std::move(out)); }
	}
	if (o.n) sink(std::move(o));
}

// ---- per-window query track -----------------------------------------------------------------------------------------------------------------
void gsah_qtrack(const HostIndex &ix, const ContigResult &r, int32_t qlen, int32_t W, std::vector<gsa_qtrack_win> &win)
{
	win.clear();
	if (r.summary || W <= 0 || qlen <= 0) return;      // (a summary result holds neither records nor strings)
	const size_t nchr = ix.chr_len.size();
	const int64_t nwin = ((int64_t)qlen + W - 1) / W;
	std::vector<uint32_t> bin;                    // {n_eq, n_x, n_ins, n_del} per window
	std::vector<std::pair<int64_t, int> > ev;     // the counted blocks' kept query intervals as (position, -1 / +1)
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		const gsa_block &b = r.blocks[bi];
		if (b.bdup != 0 || b.n_frag <= 0 || b.chr < 0 || (size_t)b.chr >= nchr) continue;
		const gsa_frag first = r.frag(b.frag_off), last = r.frag(b.frag_off + b.n_frag - 1);
		const int64_t start = first.rpos, end = last.rpos + last.rlen - extension(ix, b, last);
		if (end <= start) continue;
		if (bin.empty()) bin.assign((size_t)nwin * 4, 0u);
		std::atomic<int64_t> q1((int64_t)last.qpos + last.qlen);      // behind the last kept query base: the one record that holds the cut (if any) says where
		// a range of the block's records: the counts of one window are gathered while the walk stays in it and added when it leaves (several threads may meet in a window)
		auto piece = [&](size_t fb, size_t fe) {
			int64_t cur = -1; uint32_t cnt[4] = { 0, 0, 0, 0 };
			auto flush = [&] {
				if (cur >= 0 && cur < nwin) for (int f = 0; f < 4; f++) if (cnt[f]) __atomic_fetch_add(&bin[(size_t)cur * 4 + f], cnt[f], __ATOMIC_RELAXED);
				cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
			};
			// n columns of field f charged to the query bases q, q + 1, ... (step 0: all to q): split over the windows by arithmetic
			auto run = [&](int64_t q, int64_t n, int f, int step) {
				while (n > 0) {
					const int64_t j = q / W, m = step ? std::min<int64_t>(n, (j + 1) * W - q) : n;
					if (j != cur) { flush(); cur = j; }
					cnt[f] += (uint32_t)m; q += m; n -= m;
				}
			};
			for (size_t k = fb; k < fe; k++) {
				const gsa_frag f = r.frag(b.frag_off + (int64_t)k);
				if (f.rpos > end) break;      // (the kept columns are a prefix of the block's)
				if (f.bseed) {
					const int64_t n = std::min<int64_t>(f.qlen, end - f.rpos);
					run(f.qpos, n, 0, 1);
					if (n < f.qlen) q1.store(f.qpos + n);
					continue;
				}
				const char *x1 = r.aln1.data() + f.aln_off, *x2 = r.aln2.data() + f.aln_off;
				int64_t rp = f.rpos, qp = f.qpos;
				for (int c = 0; c < f.aln_len; c++) {
					if (x1[c] == '-') {      // an inserted query base: kept with the reference base consumed last in front of it
						if (rp > end) { q1.store(qp); break; }
						run(qp, 1, 2, 1); qp++;
						continue;
					}
					if (rp >= end) { q1.store(qp); break; }
					if (x2[c] == '-') { if (qp > 0) run(qp - 1, 1, 3, 0); }      // (a deleted base belongs to the query base consumed last)
					else { run(qp, 1, column_class(x1[c], x2[c]) == GSA_CIGAR_EQ ? 0 : 1, 1); qp++; }
					rp++;
				}
			}
			flush();
		};
		if ((size_t)b.n_frag * 16 >= par_min_bytes()) par_ranges((size_t)b.n_frag, (size_t)1 << 13, piece); else piece(0, (size_t)b.n_frag);
		const int64_t q0 = first.qpos, qe = std::min<int64_t>(q1.load(), qlen);
		if (qe > q0 && q0 >= 0) { ev.push_back({ q0, 1 }); ev.push_back({ qe, -1 }); }
	}
	if (ev.empty()) return;
	// a sweep over the sorted ends (an end in front of a start at the same position): every stretch of one depth goes to the windows it touches
	std::sort(ev.begin(), ev.end());
	struct Acc { int64_t j; uint32_t cov, multi; };
	std::vector<Acc> acc;                         // the windows under some block, ascending
	int d = 0;
	for (size_t i = 0; i + 1 < ev.size(); i++) {
		d += ev[i].second;
		int64_t s = ev[i].first; const int64_t e = ev[i + 1].first;
		while (d >= 1 && s < e) {
			const int64_t j = s / W, m = std::min<int64_t>(e, (j + 1) * W) - s;
			if (acc.empty() || acc.back().j != j) acc.push_back(Acc{ j, 0u, 0u });
			acc.back().cov += (uint32_t)m; if (d >= 2) acc.back().multi += (uint32_t)m;
			s += m;
		}
	}
	for (const auto &a : acc) {
		const int64_t lo = a.j * W, hi = std::min<int64_t>(lo + W, qlen);
		const uint32_t *c = &bin[(size_t)a.j * 4];
		gsa_qtrack_win w; w.start = (int32_t)lo; w.len = (int32_t)(hi - lo); w.n_cov = a.cov; w.n_multi = a.multi; w.n_eq = c[0]; w.n_x = c[1]; w.n_ins = c[2]; w.n_del = c[3];
		win.push_back(w);
	}
}

// <prefix>.qtrack.tsv: one line per window -- query name, BED-style start and end inside the contig, and the six counts
void Emitter::qtrack_text(bool first, const QueryContig &q, const gsa_qtrack_win *win, int64_t n_win, const std::function<void(OutBuf &&)> &sink) const
{
	OutBuf o;
	if (first) o.append("#query\tstart\tend\tcovered\tmulti\tmatch\tmismatch\tinserted\tdeleted\n");
	for (int64_t i = 0; i < n_win; i++) {
		const gsa_qtrack_win &t = win[i];
		o.reserve(o.n + q.name.size() + 128);
		char *w = o.p + o.n;
		memcpy(w, q.name.data(), q.name.size()); w += q.name.size(); *w++ = '\t';
		w = put_int(w, t.start); *w++ = '\t';
		w = put_int(w, (long long)t.start + t.len); *w++ = '\t';
		w = put_int(w, (long long)t.n_cov); *w++ = '\t';
		w = put_int(w, (long long)t.n_multi); *w++ = '\t';
		w = put_int(w, (long long)t.n_eq); *w++ = '\t';
		w = put_int(w, (long long)t.n_x); *w++ = '\t';
		w = put_int(w, (long long)t.n_ins); *w++ = '\t';
		w = put_int(w, (long long)t.n_del); *w++ = '\n';
		o.n = (size_t)(w - o.p);
		if (o.n >= ((size_t)4 << 20)) { OutBuf out = std::move(o); o = OutBuf(); sink(std::move(out)); }
	}
	if (o.n) sink(std::move(o));
}

// ---- the query projected onto the reference ------------------------------------------------------------------------------------------------
void gsah_project(const HostIndex &ix, const char *seq, const ContigResult &r, uint32_t flags, uint32_t *words, gsa_proj_stat *stat)
{
	if (stat) { stat->n_blocks = 0; stat->_pad = 0; stat->n_cols = 0; }
	if (r.summary || !words) return;      // (a summary result holds neither records nor strings)
	std::atomic<int64_t> cols(0);
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		const gsa_block &b = r.blocks[bi];
		if (b.n_frag <= 0 || (b.bdup != 0 && (flags & GSA_PROJ_NO_DUP))) continue;
		const gsa_frag first = r.frag(b.frag_off), last = r.frag(b.frag_off + b.n_frag - 1);
		const int64_t start = first.rpos, end = last.rpos + last.rlen - extension(ix, b, last);
		if (end <= start) continue;
		const bool rev = !b.bdir;
		const uint32_t key = (b.bdup == 0 ? 0x80000000u : 0u) | ((uint32_t)std::min<int64_t>(std::max<int64_t>(b.score, 0), (1 << 28) - 1) << 3);
		// a range of the block's records; several blocks (and threads) may meet in a word: the maximum is taken atomically
		auto piece = [&](size_t fb, size_t fe) {
			int64_t n = 0;
			auto offer = [&](int64_t t, uint32_t code) {
				if (t < start || t >= end) return;
				const int64_t p = rev ? 2 * ix.G - 1 - t : t;
				if (p < 0 || p >= ix.G) return;
				const uint32_t v = key | ((rev && code <= 4u) ? 5u - code : code);
				uint32_t cur = __atomic_load_n(&words[p], __ATOMIC_RELAXED);
				while (cur < v && !__atomic_compare_exchange_n(&words[p], &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
				n++;
			};
			for (size_t k = fb; k < fe; k++) {
				const gsa_frag f = r.frag(b.frag_off + (int64_t)k);
				if (f.bseed) { for (int i = 0; i < f.rlen; i++) offer(f.rpos + i, seq ? (uint32_t)nt4((unsigned char)seq[f.qpos + i]) + 1u : 5u); continue; }
				const char *x1 = r.aln1.data() + f.aln_off, *x2 = r.aln2.data() + f.aln_off;
				int64_t rp = f.rpos;
				for (int c = 0; c < f.aln_len; c++) {
					if (x1[c] == '-') continue;      // (an inserted query base has no reference base)
					offer(rp, x2[c] == '-' ? 6u : (uint32_t)nt4((unsigned char)x2[c]) + 1u);
					rp++;
				}
			}
			cols.fetch_add(n);
		};
		if ((size_t)b.n_frag * 16 >= par_min_bytes()) par_ranges((size_t)b.n_frag, (size_t)1 << 13, piece); else piece(0, (size_t)b.n_frag);
		if (stat) stat->n_blocks++;
	}
	if (stat) stat->n_cols = cols.load();
}

void gsah_proj_text(const uint32_t *words, int64_t n, char *text)
{
	static const char tab[8] = { 'n', 'A', 'C', 'G', 'T', 'N', '-', '?' };
	auto piece = [&](size_t ib, size_t ie) { for (size_t i = ib; i < ie; i++) text[i] = tab[words[i] & 7u]; };
	if (n > 0 && (size_t)n * 4 >= par_min_bytes()) par_ranges((size_t)n, (size_t)1 << 16, piece); else if (n > 0) piece(0, (size_t)n);
}

// <prefix>.proj.fa: '>' + the reference sequence's name, then the sequence's characters (text[0 .. chr_len)) 60 per line
void Emitter::proj_text(int chr, const char *text, const std::function<void(OutBuf &&)> &sink) const
{
	if (chr < 0 || (size_t)chr >= idx->chr_name.size()) return;
	const std::string &name = idx->chr_name[(size_t)chr];
	const int64_t len = idx->chr_len[(size_t)chr];
	OutBuf o;
	o.reserve((size_t)std::min<int64_t>(len + len / 60 + 2, (int64_t)5 << 20) + name.size() + 2);
	o.append(">", 1); o.append(name); o.append("\n", 1);
	for (int64_t at = 0; at < len; at += 60) {
		o.append(text + at, (size_t)std::min<int64_t>(60, len - at)); o.append("\n", 1);
		if (o.n >= ((size_t)4 << 20)) { OutBuf out = std::move(o); o = OutBuf(); sink(std::move(out)); }
	}
	if (o.n) sink(std::move(o));
}

void Emitter::aln(FILE *fp, const QueryContig &q, ContigResult &r) const
{
	std::string t1, t2;
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		gsa_block &b = r.blocks[bi];
		if (!allow_dup && b.bdup) continue;
		block_text(q, r, b, t1, t2);
		const unsigned full = (unsigned)t1.size();
		const gsa_frag last = r.frag(b.frag_off + b.n_frag - 1);
		const int ext = extension(*idx, b, last);
		if (ext > 0) { b.aln_len -= ext; b.score -= ext; r.trim(b.frag_off + b.n_frag - 1, ext); t1[b.aln_len] = t2[b.aln_len] = '\0'; }
		std::string rname = idx->chr_name[b.chr], qname = q.name;
		if (qname.size() > rname.size()) rname.append(qname.size() - rname.size(), ' '); else qname.append(rname.size() - qname.size(), ' ');
		fprintf(fp, "#Identity = %d / %d (%.2f%%) Orientation = %s\n\n", b.score, b.aln_len, (int)(1000 * (1.0 * b.score / b.aln_len)) / 10.0, b.bdir ? "Forward" : "Reverse");
		unsigned pos = 0; int qp = r.frag(b.frag_off).qpos + 1; long long rp = b.gpos;
		while (pos < full) {                                         // the reference loops over the UNtrimmed length (tools.cpp:275)
			const unsigned stop = pos + 80 > full ? full : pos + 80;
			const int p = 80 - count_gaps(t1, pos, stop), qn = 80 - count_gaps(t2, pos, stop);
			fprintf(fp, "ref.%s\t%12lld\t%.80s\nqry.%s\t%12d\t%.80s\n\n", rname.c_str(), rp, t1.c_str() + pos, qname.c_str(), qp, t2.c_str() + pos);
			pos += 80; rp += (b.bdir ? p : 0 - p); qp += qn;
		}
		fprintf(fp, "%s\n", std::string(100, '*').c_str());
	}
}

bool Emitter::dotplot(const std::string &gp_path, const std::string &out_prefix, const QueryContig &q, const ContigResult &r, std::vector<std::string> *data_files) const
{
	static const char *colors[10] = { "red", "blue", "web-green", "dark-magenta", "orange", "yellow", "turquoise", "dark-yellow", "violet", "dark-grey" };
	if (r.blocks.empty()) return false;
	const int nchr = (int)idx->chr_len.size();
	std::vector<int> sum((size_t)nchr, 0);
	for (const gsa_block &b : r.blocks) if (b.score > 0) sum[(size_t)b.chr] += b.score;
	std::vector<std::pair<int, int64_t> > top;                          // reference sequences with >= 1000 identical columns, best five
	for (int i = 0; i < nchr; i++) if (sum[(size_t)i] >= 1000) top.push_back(std::make_pair(i, (int64_t)sum[(size_t)i]));
	if (top.empty()) return false;
	std::sort(top.begin(), top.end(), [](const std::pair<int, int64_t> &a, const std::pair<int, int64_t> &b) { return a.second > b.second; });
	if (top.size() > 5) top.resize(5);
	FILE *gp = fopen(gp_path.c_str(), "w"); if (!gp) return false;
	const std::string data = out_prefix + "." + q.name;
	std::vector<FILE *> fh((size_t)nchr, (FILE *)NULL);
	for (size_t i = 0; i < top.size(); i++) {
		const std::string fn = data + "vs" + idx->chr_name[(size_t)top[i].first];
		fh[(size_t)top[i].first] = fopen(fn.c_str(), "w");
		if (fh[(size_t)top[i].first]) { fprintf(fh[(size_t)top[i].first], "0 0\n0 0\n\n"); if (data_files) data_files->push_back(fn); }
	}
	fprintf(gp, "set terminal postscript color solid 'Courier' 15\nset output '%s-%s.ps'\nset grid\nset border 1\n", out_prefix.c_str(), q.name.c_str());
	for (size_t i = 0; i < top.size(); i++) fprintf(gp, "set style line %d lw 4 pt 0 ps 0.5 lc '%s'\n", (int)i + 1, colors[i]);
	fprintf(gp, "set xrange[1:*]\nset yrange[1:*]\nset xlabel 'Query (%s)'\nset ylabel 'Ref'\n", q.name.c_str());
	fprintf(gp, "plot ");
	for (size_t i = 0; i < top.size(); i++) {
		const std::string &cn = idx->chr_name[(size_t)top[i].first];
		fprintf(gp, "'%svs%s' title '%s' with lp ls %d%s", data.c_str(), cn.c_str(), cn.c_str(), (int)i + 1, i + 1 != top.size() ? ", " : "\n\n");
	}
	for (const gsa_block &b : r.blocks) {
		if (b.score <= 0 || !fh[(size_t)b.chr]) continue;
		const gsa_frag first = r.frag(b.frag_off), last = r.frag(b.frag_off + b.n_frag - 1);
		int d, c, g0, g1;
		idx->coordinate(first.rpos, &d, &c, &g0); idx->coordinate(last.rpos + last.rlen - 1, &d, &c, &g1);
		fprintf(fh[(size_t)b.chr], "%d %d\n%d %d\n\n", first.qpos + 1, g0, last.qpos + last.qlen, g1);
	}
	for (FILE *f : fh) if (f) fclose(f);
	fclose(gp);
	return true;
}

// VariantIdentification for the records [kb, ke) of one block (SeqVariant.cpp:27-117): a record's variants depend on that record only
static void variants_of(const HostIndex *idx, int query_idx, const QueryContig &q, const ContigResult &r, const gsa_block &b, size_t kb, size_t ke, std::vector<Variant> &vars, int cnt[3])
{
	// Every allele the reference copies into a Variant (SeqVariant.cpp: ref_frag / alt_frag) is a piece of RefSequence or of the query sequence --
	// also the single columns it takes from the gapped strings, which hold exactly those bytes -- so a Variant points there instead of owning
	// two std::strings: 30 M variants of a human genome are 40 bytes each, written once.
	const char *ref = idx->ref.data(), *qs = q.seq.data();
	Variant v; v.chr_idx = b.chr; v.query_idx = query_idx;
	int d, c, g;
	for (size_t k = kb; k < ke; k++) {
		const gsa_frag f = r.frag(b.frag_off + (int64_t)k);
		if (f.bseed) continue;
		if (f.qlen == 0 && f.rlen == 0) continue;
		if (f.qlen == 0) {                                        // pure deletion (:36-45)
			cnt[2]++;
			v.type = 2; idx->coordinate(f.rpos - 1, &d, &c, &g); v.pos = g;
			v.ref_p = ref + f.rpos - 1; v.ref_n = (uint32_t)f.rlen + 1; v.alt_p = qs + f.qpos - 1; v.alt_n = 1;
			vars.push_back(v);
		} else if (f.rlen == 0) {                                 // pure insertion (:46-55)
			cnt[1]++;
			v.type = 1; idx->coordinate(f.rpos - 1, &d, &c, &g); v.pos = g;
			v.ref_p = ref + f.rpos - 1; v.ref_n = 1; v.alt_p = qs + f.qpos - 1; v.alt_n = (uint32_t)f.qlen + 1;
			vars.push_back(v);
		} else if (f.qlen == 1 && f.rlen == 1) {                  // 1x1 (:56-67)
			const char a1 = r.aln1[f.aln_off], a2 = r.aln2[f.aln_off];
			if (nt4(a1) != nt4(a2) && nt4(a2) != 4) {
				cnt[0]++;
				v.type = 0; idx->coordinate(f.rpos, &d, &c, &g); v.pos = g;
				v.ref_p = ref + f.rpos; v.ref_n = 1; v.alt_p = qs + f.qpos; v.alt_n = 1;      // (the column a1 / a2 = these two bytes)
				vars.push_back(v);
			}
		} else {                                                  // walk the aligned columns (:68-115)
			const char *x1 = r.aln1.data() + f.aln_off, *x2 = r.aln2.data() + f.aln_off;
			const int L = f.aln_len; int64_t rp = f.rpos; int qp = f.qpos;
			for (int i = 0; i < L; i++) {
				if (x1[i] == '-') {
					cnt[1]++;
					int n = 1; while (i + n < L && x1[i + n] == '-') n++;
					v.type = 1; idx->coordinate(rp - 1, &d, &c, &g); v.pos = g;
					v.ref_p = qs + qp - 1; v.ref_n = 1; v.alt_p = qs + qp - 1; v.alt_n = (uint32_t)n + 1;           // REF anchor comes from the QUERY (App. B #15)
					vars.push_back(v);
					qp += n; i += n - 1;
				} else if (x2[i] == '-') {
					cnt[2]++;
					int n = 1; while (i + n < L && x2[i + n] == '-') n++;
					v.type = 2; idx->coordinate(rp - 1, &d, &c, &g); v.pos = g;
					v.ref_p = ref + rp - 1; v.ref_n = (uint32_t)n + 1; v.alt_p = ref + rp - 1; v.alt_n = 1;
					vars.push_back(v);
					rp += n; i += n - 1;
				} else if (nt4(x1[i]) != nt4(x2[i])) {
					if (nt4(x2[i]) != 4) {
						cnt[0]++;
						v.type = 0; idx->coordinate(rp, &d, &c, &g); v.pos = g;
						v.ref_p = ref + rp; v.ref_n = 1; v.alt_p = qs + qp; v.alt_n = 1;      // (the literal column characters = these two bytes)
						vars.push_back(v);
					}
					rp++; qp++;
				} else { rp++; qp++; }
			}
		}
	}
}

// The same walk writing gsa_variant records (gsa_hip.h) in the serial order: what gsa_call_variants computes on the device, on the host -- the comparator
// of the device pass, and the variant caller of a host that holds a gsa_result and no GPU context.  Returns the number of variants (at most `cap` are stored).
int64_t gsah_variant_records(const HostIndex *idx, const ContigResult &r, gsa_variant *out, int64_t cap, int64_t counts[3])
{
	int64_t n = 0; int d, c, g;
	counts[0] = counts[1] = counts[2] = 0;
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		const gsa_block &b = r.blocks[bi];
		if (b.bdup) continue;
		auto put = [&](int kind, int64_t rpos, int qpos, int len) {
			counts[kind == 0 ? 0 : (kind == 1 || kind == 3 ? 1 : 2)]++;
			if (n < cap) { gsa_variant &v = out[n]; idx->coordinate(rpos, &d, &c, &g); v.rpos = rpos; v.qpos = qpos; v.len = len; v.chr = b.chr; v.pos = g; v.kind = kind; v.block = (int32_t)bi; }
			n++;
		};
		for (int64_t k = 0; k < b.n_frag; k++) {
			const gsa_frag f = r.frag(b.frag_off + k);
			if (f.bseed || (f.qlen == 0 && f.rlen == 0)) continue;
			if (f.qlen == 0) put(2, f.rpos - 1, f.qpos - 1, f.rlen);
			else if (f.rlen == 0) put(1, f.rpos - 1, f.qpos - 1, f.qlen);
			else if (f.qlen == 1 && f.rlen == 1) { const char a1 = r.aln1[f.aln_off], a2 = r.aln2[f.aln_off]; if (nt4(a1) != nt4(a2) && nt4(a2) != 4) put(0, f.rpos, f.qpos, 0); }
			else {
				const char *x1 = r.aln1.data() + f.aln_off, *x2 = r.aln2.data() + f.aln_off;
				const int L = f.aln_len; int64_t rp = f.rpos; int qp = f.qpos;
				for (int i = 0; i < L; i++) {
					if (x1[i] == '-') { int m = 1; while (i + m < L && x1[i + m] == '-') m++; put(3, rp - 1, qp - 1, m); qp += m; i += m - 1; }
					else if (x2[i] == '-') { int m = 1; while (i + m < L && x2[i + m] == '-') m++; put(4, rp - 1, qp - 1, m); rp += m; i += m - 1; }
					else { if (nt4(x1[i]) != nt4(x2[i]) && nt4(x2[i]) != 4) put(0, rp, qp, 0); rp++; qp++; }
				}
			}
		}
	}
	return n;
}

// VarVec from gsa_variant records (gsa_call_variants): the alleles are addressed in RefSequence / the query, as Emitter::variants leaves them
void Emitter::variants_from(int query_idx, const QueryContig &q, const gsa_variant *v, int64_t n)
{
	static const int type_of[5] = { 0, 1, 2, 1, 2 };
	const char *ref = idx->ref.data(), *qs = q.seq.data();
	const size_t per = (size_t)1 << 20;
	for (int64_t at = 0; at < n; at += (int64_t)per) {
		const size_t m = (size_t)std::min<int64_t>((int64_t)per, n - at);
		var_chunks.emplace_back();
		std::vector<Variant> &vc = var_chunks.back(); vc.resize(m);
		auto one = [&](size_t j0, size_t j1) {
			for (size_t j = j0; j < j1; j++) {
				const gsa_variant &g = v[at + (int64_t)j]; Variant &o = vc[j];
				o.pos = g.pos; o.chr_idx = g.chr; o.query_idx = query_idx; o.type = type_of[g.kind >= 0 && g.kind < 5 ? g.kind : 0];      // (kinds are 0..4 by construction; a record from elsewhere must not index past the table)
				gsa_variant_alleles(&g, ref, qs, &o.ref_p, &o.ref_n, &o.alt_p, &o.alt_n);
			}
		};
		const size_t parts = m * sizeof(Variant) < par_min_bytes() ? 1 : (size_t)HostPool::global().threads();
		if (parts <= 1) one(0, m); else HostPool::global().run(parts, [&](size_t k) { one(m * k / parts, m * (k + 1) / parts); });
		for (size_t j = 0; j < m; j++) { const int t = vc[j].type; if (t == 0) n_snv++; else if (t == 1) n_ins++; else n_del++; }
	}
}

// VarVec grows block after block, record after record (SeqVariant.cpp:12-119); here a long block's records are dealt to the pool in ranges
// and the ranges' lists are kept IN THAT ORDER (var_chunks): the sequence the final sort sees is the serial one.
void Emitter::variants(int query_idx, const QueryContig &q, ContigResult &r)
{
	for (size_t bi = 0; bi < r.blocks.size(); bi++) {
		const gsa_block &b = r.blocks[bi];
		if (b.bdup) continue;
		const size_t nf = (size_t)b.n_frag;
		if (nf * 16 < par_min_bytes()) {
			if (var_chunks.empty() || var_chunks.back().size() > ((size_t)1 << 20)) var_chunks.emplace_back();
			int cnt[3] = { 0, 0, 0 };
			variants_of(idx, query_idx, q, r, b, 0, nf, var_chunks.back(), cnt);
			n_snv += cnt[0]; n_ins += cnt[1]; n_del += cnt[2];
			continue;
		}
		const size_t parts = std::min<size_t>((size_t)HostPool::global().threads() * 4, nf / 4096 + 1);
		const size_t at = var_chunks.size();
		var_chunks.resize(at + parts);
		std::vector<std::array<int, 3> > cnts(parts, std::array<int, 3>{ { 0, 0, 0 } });
		HostPool::global().run(parts, [&](size_t k) {
			variants_of(idx, query_idx, q, r, b, nf * k / parts, nf * (k + 1) / parts, var_chunks[at + k], cnts[k].data());
		});
		for (size_t k = 0; k < parts; k++) { n_snv += cnts[k][0]; n_ins += cnts[k][1]; n_del += cnts[k][2]; }
	}
}

// OutputSequenceVariants (SeqVariant.cpp:121-143).  The reference std::sorts VarVec on (chr_idx, pos) -- an incomplete key: the order of
// variants that share a position is whatever libstdc++'s introsort leaves (App. B #17).  What introsort does depends on the comparator's
// answers only, never on what else an element carries, so sorting 16-byte keys {chr, pos, where the variant lies} with the same comparator
// on the same initial sequence makes the same comparisons and the same moves: the permutation is the reference's, without dragging two
// std::strings per element through every swap; and introsort's partition steps split the array into parts that never meet again, so they run
// on the pool's threads (exact_sort.h: std::sort's permutation, element for element).  The lines are then formatted by the pool in ranges and
// written in order.
void Emitter::vcf_text(const std::string &reference_label, const std::function<void(OutBuf &&)> &sink)
{
	static const char *MutType[3] = { "SUBSTITUTE", "INSERT", "DELETE" };
	struct Key { int32_t chr, pos; uint32_t chunk, at; };
	struct ByPos { bool operator()(const Key &a, const Key &b) const { return a.chr == b.chr ? a.pos < b.pos : a.chr < b.chr; } };
	if (!vars.empty()) { var_chunks.insert(var_chunks.begin(), std::vector<Variant>()); var_chunks.front().swap(vars); }      // (variants pushed into `vars` directly come first)
	std::vector<size_t> base(var_chunks.size() + 1, 0);
	for (size_t c = 0; c < var_chunks.size(); c++) base[c + 1] = base[c] + var_chunks[c].size();
	const size_t n = base.back();
	std::vector<Key> keys(n);
	HostPool::global().run(var_chunks.size(), [&](size_t c) {
		const std::vector<Variant> &vc = var_chunks[c]; Key *k = keys.data() + base[c];
		for (size_t i = 0; i < vc.size(); i++) { k[i].chr = vc[i].chr_idx; k[i].pos = vc[i].pos; k[i].chunk = (uint32_t)c; k[i].at = (uint32_t)i; }
	});
	exact_sort(keys.data(), keys.data() + keys.size(), ByPos());      // std::sort's permutation (same incomplete key, same initial order), on the pool: exact_sort.h
	{
		OutBuf h;
		h.append("##fileformat=VCFv4.1\n"); h.append("##reference=" + reference_label + "\n"); h.append("##source=GSAlign 1.0.22\n");
		h.append("##INFO=<ID=TYPE,Number=1,Type=String,Description=\"The type of allele, either SUBSTITUTE, INSERT, or DELETE.\">\n");
		for (size_t i = 0; i < idx->chr_name.size(); i++) h.append("##contig=<ID=" + idx->chr_name[i] + ",length=" + std::to_string(idx->chr_len[i]) + ">\n");
		h.append("#CHROM	POS	ID	REF	ALT	QUAL	FILTER	INFO\n");
		sink(std::move(h));
	}
	const size_t per = (size_t)1 << 16, parts = (n + per - 1) / per;
	// (ranges are formatted a batch at a time so that the writer gets them in order while the next batch is formatted)
	const size_t batch = (size_t)HostPool::global().threads() * 2;
	for (size_t p0 = 0; p0 < parts; p0 += batch) {
		const size_t pn = std::min(batch, parts - p0);
		std::vector<OutBuf> outs(pn);
		auto one = [&](size_t j) {
			const size_t b = (p0 + j) * per, e = std::min(n, b + per);
			OutBuf &o = outs[j]; o.reserve((e - b) * 48);
			for (size_t i = b; i < e; i++) {
				const Variant &v = var_chunks[keys[i].chunk][keys[i].at];
				const std::string &cn = idx->chr_name[(size_t)v.chr_idx];
				const char *mt = MutType[v.type]; const size_t ml = strlen(mt);
				const size_t rl = v.ref_n, al = v.alt_n;      // (RefSequence and a validated query hold no NUL: "%s" prints the whole fragment)
				const size_t need = cn.size() + rl + al + ml + 48;
				if (o.n + need > o.cap) o.reserve((o.n + need) * 2);
				char *w = o.p + o.n;
				memcpy(w, cn.data(), cn.size()); w += cn.size(); *w++ = '\t';
				w = put_int(w, v.pos); memcpy(w, "\t.\t", 3); w += 3;
				memcpy(w, v.ref_p, rl); w += rl; *w++ = '\t';
				memcpy(w, v.alt_p, al); w += al;
				memcpy(w, "\t100\t*\tTYPE=", 12); w += 12;
				memcpy(w, mt, ml); w += ml; *w++ = '\n';
				o.n = (size_t)(w - o.p);
			}
		};
		if (n * 48 < par_min_bytes()) for (size_t j = 0; j < pn; j++) one(j); else HostPool::global().run(pn, one);
		for (size_t j = 0; j < pn; j++) sink(std::move(outs[j]));
	}
}

void Emitter::vcf(FILE *fp, const std::string &reference_label)
{
	vcf_text(reference_label, [&](OutBuf &&o) { if (o.n) fwrite(o.p, 1, o.n, fp); });
}
