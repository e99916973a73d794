// Tax annotate and consensus verbs, and the glue that binds a sequence database to a taxonomy.
//
//   pgx_taxcollect_file     `perl NCBI-taxcollector-0.01.pl -f in -o out` (NCBI-taxcollector-0.01.pl:20-164):
//                           host parses the hit table, ONE kernel walks every gi (taxdb.hip), host renders
//                           the lineage text with the driver's digit / underscore rules (taxcollector:96-144)
//   pgx_db_bind_taxonomy    the same walk once per database subject; lineage text and consensus tokens
//                           stay in HBM for the fused pipeline
//   pgx_consensus_file      `perl Consensus_BLAST_SOAP_RDP-1.1.pl -b -r [-s] -o` (Consensus:8-244): the cursor
//                           logic over the two files is control flow on ids (host); agreement counting and
//                           the order-dependent arg-max run on the device (consensus_core.hpp)
#include <algorithm>
#include <functional>
#include <chrono>
#include <map>

#include "bitops.hpp"
#include "consensus_core.hpp"
#include <mutex>
#include <tuple>
#include <thread>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "engine.hpp"
#include "taxdb.hpp"

namespace pgx {

bool consensus_format_pieces(const pgx_db *db, const pgx_reads *reads, const pgx_hits *hits, const pgx_consensus_rec *recs, int64_t n,
			     uint64_t piece, const std::function<int(const char *, size_t)> &sink, int *rc_out);
bool consensus_format_device(const pgx_db *db, const pgx_reads *reads, const pgx_hits *hits, const pgx_consensus_rec *recs, int64_t n,
			     std::string &out, int *rc_out);
int formatter_tables(const pgx_db *db);
void format_hit_columns(const pgx_hit &h, int64_t qlen, int64_t db_len, int64_t db_nseq, bool gapped, Text &out);

// ------------------------------------------------------------------------------------------ lineage text
LineageRenderer::~LineageRenderer() { delete cache; }

// "[idx]" followed by "name;|" when `tax_class -n` yields a scientific name (taxcollector:264-273)
std::string LineageRenderer::piece(int32_t taxid)
{
	if (!cache)
		cache = new std::unordered_map<int32_t, std::string>();
	auto it = cache->find(taxid);
	if (it != cache->end())
		return it->second;
	pgx_node nd;
	tax_node_record(db, taxid, &nd);
	char idx[16];
	snprintf(idx, sizeof idx, "[%d]", (int)driver_rank_code(nd.rank));
	std::string s = idx, name;
	if (tax_scientific_name(db, taxid, name))
		s += name + ";|";
	(*cache)[taxid] = s;
	return s;
}

static inline bool perl_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }

std::string LineageRenderer::render(const int32_t *lineage, int count, int status, const std::string &gi_text)
{
	std::string cat;
	if (status == 1) {
		cat = "Unidentified(GI:" + gi_text + ");|";
	} else {
		for (int k = 0; k < count; k++)
			cat += lineage[k] == PGX_LIN_UNCLASSIFIED ? std::string("[0]Unclassified;|") : piece(lineage[k]);
	}
	// split on '|', trailing empty elements dropped (taxcollector:96-97)
	std::vector<std::string> el;
	size_t s = 0;
	while (s <= cat.size()) {
		size_t bar = cat.find('|', s);
		if (bar == std::string::npos)
			bar = cat.size();
		el.emplace_back(cat, s, bar - s);
		if (bar == cat.size())
			break;
		s = bar + 1;
	}
	while (!el.empty() && el.back().empty())
		el.pop_back();
	bool any5 = false;
	for (auto &e : el)
		if (e.find('5') != std::string::npos)
			any5 = true;
	std::string out;
	for (size_t i = el.size(); i-- > 0;) {
		std::string e = el[i];
		size_t six = e.find('6');
		if (six != std::string::npos) {
			// species branch (taxcollector:109-126): blanks -> '_'; without any '5' print the element
			// twice, first with its first '6' turned into '5'
			for (auto &c : e)
				if (perl_space(c))
					c = '_';
			if (!any5) {
				e[six] = '5';
				out += e;
				e[six] = '6';
			}
			out += e;
		} else {
			size_t sev = e.find('7');
			if (sev != std::string::npos)
				e[sev] = '9'; // taxcollector:130-134
			out += e;
		}
	}
	return out;
}

// split(/\ |\t\t|\t/, line): leading empty fields kept, trailing dropped (taxcollector:77)
static void split_columns(const std::string &line, std::vector<std::string> &f)
{
	f.clear();
	size_t s = 0, i = 0;
	while (i < line.size()) {
		int sep = 0;
		if (line[i] == ' ')
			sep = 1;
		else if (line[i] == '\t')
			sep = (i + 1 < line.size() && line[i + 1] == '\t') ? 2 : 1;
		if (sep) {
			f.emplace_back(line, s, i - s);
			i += sep;
			s = i;
		} else {
			i++;
		}
	}
	f.emplace_back(line, s, line.size() - s);
	while (!f.empty() && f.back().empty())
		f.pop_back();
}

// the same line straight from the text: fields of split(/\ |\t\t|\t/) are walked in place (no per-field strings)
static void emit_collected_fast(const char *line, size_t n, const std::string &lineage, std::string &out)
{
	// trailing empty fields are dropped by the split, which only matters for which indices exist: empty fields are
	// never printed anyway
	size_t s = 0, i = 0;
	int field = 0;
	auto flush = [&](size_t e) {
		if (field == 0) {
			out.append(line + s, e - s);
			out += '\t';
			out += lineage;
		} else if (field >= 2 && field <= 12 && e > s) {
			out += '\t';
			out.append(line + s, e - s);
		}
		field++;
	};
	while (i < n) {
		int sep = 0;
		if (line[i] == ' ')
			sep = 1;
		else if (line[i] == '\t')
			sep = (i + 1 < n && line[i + 1] == '\t') ? 2 : 1;
		if (sep) {
			flush(i);
			i += sep;
			s = i;
		} else {
			i++;
		}
	}
	flush(n);
	out += '\n';
}

// one output line of the driver: id, lineage, then input columns 2..12 that are not empty
static void emit_collected(const std::string &line, const std::string &lineage, std::string &out)
{
	std::vector<std::string> f;
	split_columns(line, f);
	if (!f.empty())
		out += f[0];
	out += '\t';
	out += lineage;
	for (size_t i = 2; i <= 12 && i < f.size(); i++)
		if (!f[i].empty()) {
			out += '\t';
			out += f[i];
		}
	out += '\n';
}

// text between the first and second '|' (taxcollector:75,84); false when the line has no '|'
static bool gi_text_of(const std::string &line, std::string &gi)
{
	size_t a = line.find('|');
	if (a == std::string::npos)
		return false;
	size_t b = line.find('|', a + 1);
	gi = line.substr(a + 1, b == std::string::npos ? std::string::npos : b - a - 1);
	return true;
}

uint32_t intern_into(std::unordered_map<std::string, uint32_t> &map, std::vector<std::string> &text, const std::string &s)
{
	auto it = map.find(s);
	if (it != map.end())
		return it->second;
	uint32_t id = (uint32_t)text.size();
	text.push_back(s);
	map.emplace(s, id);
	return id;
}

// Consensus:116-122: split on '[', ']', ';', join with blanks, split on whitespace
static void lineage_tokens(const std::string &tax, std::vector<std::string> &tok)
{
	tok.clear();
	size_t i = 0;
	auto delim = [](char c) { return perl_space(c) || c == '[' || c == ']' || c == ';'; };
	while (i < tax.size()) {
		while (i < tax.size() && delim(tax[i]))
			i++;
		size_t s = i;
		while (i < tax.size() && !delim(tax[i]))
			i++;
		if (i > s)
			tok.emplace_back(tax, s, i - s);
	}
}

static int8_t blast_rank_index(const std::string &t)
{
	return (t.size() == 1 && t[0] >= '0' && t[0] <= '6') ? (int8_t)(t[0] - '0') : (int8_t)-1;
}

// similarity strings -> ranks of their byte order ("" and "0" always present: the start values of
// $blastsim, Consensus:86-92 and :231)
static void build_sim_ranks(std::vector<std::string> uniq, std::map<std::string, uint32_t> &rank)
{
	uniq.push_back("");
	uniq.push_back("0");
	std::sort(uniq.begin(), uniq.end());
	uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
	for (size_t i = 0; i < uniq.size(); i++)
		rank[uniq[i]] = (uint32_t)i;
}

// ------------------------------------------------------------------------------------------ kernels
// one lane per group of consecutive hit lines (file verb) — hits are already in table order
__global__ void k_consensus_groups(const uint32_t *__restrict__ g_first, const uint32_t *__restrict__ g_count,
				   const uint32_t *__restrict__ g_rdp, const uint32_t *__restrict__ g_initsim, uint32_t n_groups,
				   const uint32_t *__restrict__ tok_off, const uint32_t *__restrict__ tok,
				   const int8_t *__restrict__ tok_rank, const uint32_t *__restrict__ simrank,
				   const uint32_t *__restrict__ rdp_off, const uint32_t *__restrict__ rdp_name,
				   const int8_t *__restrict__ rdp_rank, pgx_consensus_rec *__restrict__ recs)
{
	uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= n_groups)
		return;
	const uint32_t first = g_first[g], n = g_count[g], rl = g_rdp[g];
	const uint32_t r0 = rdp_off[rl], r1 = rdp_off[rl + 1];
	ArgmaxState am;
	am.cursim = g_initsim[g];
	for (uint32_t k = 0; k < n; k++) {
		const uint32_t line = first + k, t0 = tok_off[line], nt = tok_off[line + 1] - t0;
		const uint32_t rm = rank_matches(tok + t0, nt, tok_rank, rdp_name, rdp_rank, r0, r1);
		am.step((int32_t)line, rm, nt, simrank[line]);
	}
	recs[g].hit = am.win;
	recs[g].matches = (int32_t)am.maxrm;
}

// synthetic RDP stream: 6 fixed slots per read (domain..genus); a dropped rank gets a name id and a
// rank index that equal nothing
__global__ void k_synth_rdp(uint64_t read_seed, uint64_t n_seq, uint32_t seq_len, uint32_t read_len, uint64_t first,
			    uint64_t count, const int64_t *__restrict__ level_cnt, const int64_t *__restrict__ level_base,
			    const uint32_t *__restrict__ node_name_tok, uint32_t *__restrict__ name, int8_t *__restrict__ rank,
			    uint32_t *__restrict__ code)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count)
		return;
	const uint64_t r = first + i;
	const uint64_t u = synth_hash(read_seed, 3, r, 0);
	(void)seq_len;
	(void)read_len;
	int64_t idx = (int64_t)((u & 0xFFFFFFFFull) % n_seq); // species index = source sequence
	int64_t anc[6];
	for (int l = 5; l >= 0; l--) {
		idx = (int64_t)(((unsigned __int128)idx * (uint64_t)level_cnt[l]) / (uint64_t)level_cnt[l + 1]);
		anc[l] = idx;
	}
	for (int k = 0; k < 6; k++) {
		const bool keep = synth_hash(read_seed, 5, r, (uint64_t)k) % 10 != 0;
		const int64_t taxid = level_base[k] + anc[k];
		const uint32_t nm = keep ? node_name_tok[taxid] : 0xFFFFFFFFu;
		name[i * 6 + k] = nm;
		rank[i * 6 + k] = keep ? (int8_t)k : (int8_t)-2;
		code[i * 6 + k] = keep ? ((nm << 3) | (uint32_t)(k + 1)) : 0xFFFFFFFFu;
	}
}

} // namespace pgx

using namespace pgx;

uint32_t pgx_db::intern(const std::string &s) { return intern_into(token_id, token_text, s); }

extern "C" {

int pgx_taxcollect_file(pgx_taxdb *db, const char *in_path, const char *out_path, char **report_text)
{
	Text report;
	return with_text(report, report_text, [&]() -> int {
		if (!db || !in_path || !out_path)
			return fail(PGX_E_ARG, "taxcollector: -f and -o are required");
		PGX_TRY(require_device());
		bool ok;
		std::string text = read_text_file(in_path, &ok);
		if (!ok) {
			report.printf("Error: Unable to open classification results file %s.\n", in_path); // taxcollector:31-34
			return fail(PGX_E_IO, "cannot open %s", in_path);
		}
		// pass 1 (host): lines up to the first empty one (taxcollector:83-87) and where their gi texts are; nothing is copied
		struct LineRef {
			size_t s, n, g, gn; // line start/length, gi text start/length
		};
		std::vector<LineRef> lines;
		std::vector<int32_t> gi_num;
		int hang_line = -1;
		for (size_t s = 0; s < text.size();) {
			const char *nl = (const char *)memchr(text.data() + s, '\n', text.size() - s);
			const size_t e = nl ? (size_t)(nl - text.data()) : text.size();
			const char *line = text.data() + s;
			const size_t n = e - s;
			bool only_bars = true;
			for (size_t k = 0; k < n && only_bars; k++)
				only_bars = line[k] == '|';
			if (only_bars)
				break;
			const char *b1 = (const char *)memchr(line, '|', n);
			size_t g = 0, gn = 0;
			if (b1) {
				g = (size_t)(b1 - line) + 1;
				const char *b2 = (const char *)memchr(line + g, '|', n - g);
				gn = b2 ? (size_t)(b2 - line) - g : n - g;
			}
			if (!b1 || gn == 0) {
				hang_line = (int)lines.size();
				break; // `./tax_class -s` without an id: the reference recurses forever
			}
			lines.push_back({ s, n, s + g, gn });
			gi_num.push_back(atoi(std::string(line + g, gn).c_str()));
			s = e + 1;
		}
		// pass 2 (device): one walk per line
		const size_t n = lines.size();
		std::vector<int32_t> lin(n * PGX_LINEAGE_SLOTS), cnt(n), st(n), leaf(n);
		if (n) {
			DevBuf<int32_t> d_gi, d_lin, d_cnt, d_st, d_leaf;
			PGX_TRY(d_gi.assign(gi_num));
			PGX_TRY(d_lin.alloc(n * PGX_LINEAGE_SLOTS, 0, 0, true));
			PGX_TRY(d_cnt.alloc(n));
			PGX_TRY(d_st.alloc(n));
			PGX_TRY(d_leaf.alloc(n));
			PGX_TRY(tax_walk_device(db, d_gi.data(), (int64_t)n, d_lin.data(), d_cnt.data(), d_st.data(), d_leaf.data()));
			PGX_TRY(d_lin.download(lin.data(), lin.size()));
			PGX_TRY(d_cnt.download(cnt.data(), n));
			PGX_TRY(d_st.download(st.data(), n));
			PGX_TRY(d_leaf.download(leaf.data(), n));
		}
		// the driver stops at the first line whose walk never ends (or is too long for this build)
		size_t stop_at = n;
		int status = 0;
		for (size_t i = 0; i < n; i++)
			if (st[i] == 2 || st[i] == 3) {
				stop_at = i;
				const std::string g(text, lines[i].g, lines[i].gn);
				status = st[i] == 2 ? fail(PGX_E_REFHANG, "line %zu (GI %s): the reference driver never terminates on this taxonomy walk", i + 1, g.c_str())
						    : fail(PGX_E_LIMIT, "line %zu: lineage longer than %d elements", i + 1, PGX_LINEAGE_SLOTS);
				break;
			}
		// pass 3 (host, all cores): text.  Lines are independent; every worker renders a contiguous block with its own
		// name cache and remembers the lineage text per gi, the blocks are joined in order.
		const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
		const unsigned workers = (unsigned)std::max<size_t>(1, std::min<size_t>(hw, stop_at / 20000 + 1));
		std::vector<std::string> outs(workers), reps(workers);
		auto work = [&](unsigned w) {
			const size_t i0 = stop_at * w / workers, i1 = stop_at * (w + 1) / workers;
			LineageRenderer ren(db);
			std::unordered_map<std::string, std::string> memo;
			std::string &o = outs[w], &r = reps[w];
			o.reserve((i1 - i0) * 160);
			r.reserve((i1 - i0) * 64);
			char buf[96];
			for (size_t i = i0; i < i1; i++) {
				const std::string g(text, lines[i].g, lines[i].gn);
				if (st[i] == 1) {
					r += "Searching upper node for TAXID 0\n.\n"; // taxcollector:176 with "0\n"
					r += "\n\nTAXID zero GI = " + g + ".\n\n";
				} else {
					const int k = snprintf(buf, sizeof buf, "Searching upper node for TAXID %d.\nDone for TAXID %d.\n", leaf[i], leaf[i]);
					r.append(buf, (size_t)k);
				}
				auto it = memo.find(g);
				if (it == memo.end())
					it = memo.emplace(g, ren.render(&lin[i * PGX_LINEAGE_SLOTS], cnt[i], st[i], g)).first;
				emit_collected_fast(text.data() + lines[i].s, lines[i].n, it->second, o);
			}
		};
		if (workers == 1) {
			work(0);
		} else {
			std::vector<std::thread> th;
			for (unsigned w = 0; w < workers; w++)
				th.emplace_back(work, w);
			for (auto &t : th)
				t.join();
		}
		std::string out;
		size_t total_out = 0, total_rep = 0;
		for (unsigned w = 0; w < workers; w++) {
			total_out += outs[w].size();
			total_rep += reps[w].size();
		}
		out.reserve(total_out);
		report.s.reserve(report.s.size() + total_rep);
		for (unsigned w = 0; w < workers; w++) {
			out += outs[w];
			report.s += reps[w];
			std::string().swap(outs[w]);
			std::string().swap(reps[w]);
		}
		if (status == 0 && hang_line >= 0)
			status = fail(PGX_E_REFHANG, "line %d has no gi|N| subject id: the reference driver never terminates on it", hang_line + 1);
		int wrc = write_text_file(out_path, out);
		if (wrc < 0) {
			report.printf("Error: Unable to open output file %s.\n", out_path);
			return wrc;
		}
		return status;
	});
}

int pgx_db_bind_taxonomy(pgx_db *db, pgx_taxdb *tax)
{
	if (!db || !tax)
		return fail(PGX_E_ARG, "pgx_db_bind_taxonomy: null argument");
	PGX_TRY(require_device());
	const size_t n = (size_t)db->n_seq;
	std::vector<int32_t> gi(n);
	std::vector<std::string> gi_text(n);
	for (size_t i = 0; i < n; i++) {
		if (!gi_text_of(db->ids[i], gi_text[i]) || gi_text[i].empty())
			return fail(PGX_E_REFHANG, "subject %s has no gi|N| id: the reference driver cannot annotate it", db->ids[i].c_str());
		gi[i] = atoi(gi_text[i].c_str());
	}
	std::vector<int32_t> lin(n * PGX_LINEAGE_SLOTS), cnt(n), st(n), leaf(n);
	{
		DevBuf<int32_t> d_gi, d_lin, d_cnt, d_st, d_leaf;
		PGX_TRY(d_gi.alloc(n));
		PGX_TRY(d_lin.alloc(n * PGX_LINEAGE_SLOTS, 0, 0, true));
		PGX_TRY(d_cnt.alloc(n));
		PGX_TRY(d_st.alloc(n));
		PGX_TRY(d_leaf.alloc(n));
		PGX_TRY(d_gi.upload(gi.data(), n));
		PGX_TRY(tax_walk_device(tax, d_gi.data(), (int64_t)n, d_lin.data(), d_cnt.data(), d_st.data(), d_leaf.data()));
		PGX_TRY(d_lin.download(lin.data(), lin.size()));
		PGX_TRY(d_cnt.download(cnt.data(), n));
		PGX_TRY(d_st.download(st.data(), n));
		PGX_TRY(d_leaf.download(leaf.data(), n));
	}
	LineageRenderer ren(tax);
	db->lineage.assign(n, std::string());
	db->subj_taxid.assign(n, 0);
	db->token_text.clear();
	db->token_id.clear();
	db->intern(""); // id 0 = the empty string (what an undefined name compares as)
	std::vector<uint32_t> off(n + 1, 0), toks;
	toks.reserve(n * 14);
	std::vector<std::string> tk;
	for (size_t i = 0; i < n; i++) {
		if (st[i] >= 2)
			return fail(PGX_E_REFHANG, "subject %s: the reference driver never terminates on its taxonomy walk", db->ids[i].c_str());
		db->lineage[i] = ren.render(&lin[i * PGX_LINEAGE_SLOTS], cnt[i], st[i], gi_text[i]);
		db->subj_taxid[i] = leaf[i];
		lineage_tokens(db->lineage[i], tk);
		for (auto &t : tk)
			toks.push_back(db->intern(t));
		off[i + 1] = (uint32_t)toks.size();
	}
	db->h_tok_rank.resize(db->token_text.size());
	for (size_t t = 0; t < db->token_text.size(); t++)
		db->h_tok_rank[t] = blast_rank_index(db->token_text[t]);
	PGX_TRY(db->d_subj_tok_off.alloc(n + 1));
	PGX_TRY(db->d_subj_tok_off.upload(off.data(), n + 1));
	PGX_TRY(db->d_subj_tok.alloc(toks.size() ? toks.size() : 1));
	PGX_TRY(db->d_subj_tok.upload(toks.data(), toks.size()));
	PGX_TRY(db->d_tok_rank.alloc(db->h_tok_rank.size()));
	PGX_TRY(db->d_tok_rank.upload(db->h_tok_rank.data(), db->h_tok_rank.size()));
	{
		// two passes: the widest record decides the stride (8 words = 32 bytes for up to 7 pairs, else 16)
		db->max_pairs = 0;
		for (size_t i = 0; i < n; i++) {
			const uint32_t nt = off[i + 1] - off[i], np = (nt + 1) / 2;
			if (!(np > 15 || nt > 0xFFFF))
				db->max_pairs = std::max(db->max_pairs, (int)np);
		}
		const size_t W = db->max_pairs <= 7 ? 8 : 16;
		db->pair_words = (int)W;
		std::vector<uint32_t> pairs(n * W, 0);
		for (size_t i = 0; i < n; i++) {
			const uint32_t t0 = off[i], nt = off[i + 1] - t0, np = (nt + 1) / 2;
			uint32_t *rec = &pairs[i * W];
			if (np > 15 || nt > 0xFFFF) {
				rec[0] = (nt & 0xFFFF) | (0xFFFFu << 16);
				continue;
			}
			rec[0] = nt | (np << 16);
			for (uint32_t a = 0; a < np; a++) {
				const uint32_t rk = (uint32_t)(db->h_tok_rank[toks[t0 + 2 * a]] + 1);
				const uint32_t nm = 2 * a + 1 < nt ? toks[t0 + 2 * a + 1] : 0u;
				rec[1 + a] = (nm << 3) | rk;
			}
		}
		PGX_TRY(db->d_subj_pairs.alloc(pairs.size() ? pairs.size() : 16));
		PGX_TRY(db->d_subj_pairs.upload(pairs.data(), pairs.size()));
	}
	// similarity order of every "%.2f" text from 0.00 to 100.00, plus "" and "0"
	std::vector<std::string> sims;
	char buf[16];
	for (int h = 0; h <= 10000; h++) {
		snprintf(buf, sizeof buf, "%d.%02d", h / 100, h % 100);
		sims.emplace_back(buf);
	}
	std::map<std::string, uint32_t> rank;
	build_sim_ranks(sims, rank);
	std::vector<uint32_t> lut(10001);
	for (int h = 0; h <= 10000; h++)
		lut[(size_t)h] = rank[sims[(size_t)h]];
	db->simrank_undef = rank[""];
	db->simrank_zero = rank["0"];
	PGX_TRY(db->d_simrank_lut.alloc(lut.size()));
	PGX_TRY(db->d_simrank_lut.upload(lut.data(), lut.size()));
	{
		// short alignments: skip the divisions, one table read gives the rank of the pident text
		std::vector<uint32_t> byl(256 * 256, 0);
		for (int len = 1; len < 256; len++)
			for (int mm = 0; mm <= len; mm++)
				byl[(size_t)len * 256 + (size_t)mm] = lut[(size_t)pident_hundredths(len - mm, len)];
		PGX_TRY(db->d_simrank_len.alloc(byl.size()));
		PGX_TRY(db->d_simrank_len.upload(byl.data(), byl.size()));
	}
	// taxid -> token id of its cleaned scientific name (what an RDP assignment of that node would carry)
	std::vector<uint32_t> nn(tax->n_nodes + 1, 0);
	{
		// only the nodes that occur in a bound lineage matter
		std::vector<uint8_t> seen(tax->n_nodes + 1, 0);
		for (size_t i = 0; i < n; i++)
			for (int k = 0; k < cnt[i]; k++) {
				int32_t t = lin[i * PGX_LINEAGE_SLOTS + k];
				if (t > 0 && (size_t)t <= tax->n_nodes && !seen[(size_t)t]) {
					seen[(size_t)t] = 1;
					std::string name;
					if (tax_scientific_name(tax, t, name))
						nn[(size_t)t] = db->intern(clean_rdp_name(name));
				}
			}
	}
	PGX_TRY(db->d_node_name_tok.alloc(nn.size()));
	PGX_TRY(db->d_node_name_tok.upload(nn.data(), nn.size()));
	{
		// OTU ids for megaclust: one per distinct lineage text, plus one for the empty text of an empty line
		std::unordered_map<std::string, uint32_t> lin_id;
		std::vector<uint32_t> subj_lin(n);
		std::lock_guard<std::mutex> fmt_lock(db->fmt_mu);
		db->lin_blob_ready = false; // (the formatters' copy of these texts in HBM is made again at its next use)
		db->lin_text.clear();
		for (size_t i = 0; i < n; i++)
			subj_lin[i] = intern_into(lin_id, db->lin_text, db->lineage[i]);
		db->empty_lin = intern_into(lin_id, db->lin_text, std::string());
		PGX_TRY(db->d_subj_lin.alloc(n ? n : 1));
		PGX_TRY(db->d_subj_lin.upload(subj_lin.data(), n));
	}
	db->bound = true;
	PGX_TRY(formatter_tables(db)); // the lineage texts in HBM, for the consensus text (blast_format.hip)
	index_check(db, "bind_taxonomy");
	return 0;
}

const char *pgx_db_subject_lineage(const pgx_db *db, int64_t subject)
{
	if (!db || !db->bound || subject < 0 || subject >= db->n_seq)
		return nullptr;
	return db->lineage[(size_t)subject].c_str();
}

void pgx_rdp_close(pgx_rdp *r) { delete r; }

// The RDP assignments of a batch as the classifier's text (Consensus:126-132: id, five tabs, then name / rank /
// confidence in threes).  Reading the file back with pgx_rdp_from_file gives the same assignments.
int pgx_rdp_write_file(const pgx_rdp *rdp, const pgx_reads *reads, const pgx_db *db, const char *path)
{
	if (!rdp || !reads || !db || !path || rdp->n != reads->n)
		return fail(PGX_E_ARG, "pgx_rdp_write_file: bad argument");
	return pgx::guard("pgx_rdp_write_file", [&]() -> int {
		const size_t n = (size_t)rdp->n;
		std::vector<uint32_t> off(n + 1);
		PGX_TRY(rdp->d_off.download(off.data(), n + 1));
		std::vector<uint32_t> name(off[n] ? off[n] : 1);
		std::vector<int8_t> rank(off[n] ? off[n] : 1);
		std::vector<uint8_t> present(n ? n : 1);
		PGX_TRY(rdp->d_name.download(name.data(), off[n]));
		PGX_TRY(rdp->d_rank.download(rank.data(), off[n]));
		PGX_TRY(rdp->d_present.download(present.data(), n));
		static const char *const kRank[7] = { "domain", "phylum", "class", "order", "family", "genus", "species" };
		FILE *f = fopen(path, "wb");
		if (!f)
			return fail(PGX_E_IO, "cannot open %s for writing", path);
		std::string out;
		out.reserve(64u << 20);
		bool ok = true;
		for (size_t r = 0; r < n && ok; r++) {
			if (!present[r])
				continue;
			out += reads->name_of((int64_t)r);
			out += "\t\t\t\t\t";
			for (uint32_t t = off[r]; t < off[r + 1]; t++) {
				if (t > off[r])
					out += '\t';
				out += name[t] < db->token_text.size() ? db->token_text[name[t]] : std::string();
				out += '\t';
				out += rank[t] >= 0 && rank[t] < 7 ? kRank[rank[t]] : "norank";
				out += "\t0.90";
			}
			out += '\n';
			if (out.size() > (60u << 20)) {
				ok = fwrite(out.data(), 1, out.size(), f) == out.size();
				out.clear();
			}
		}
		ok = ok && fwrite(out.data(), 1, out.size(), f) == out.size();
		if (fclose(f) != 0 || !ok)
			return fail(PGX_E_IO, "short write to %s", path);
		return 0;
	});
}

int pgx_rdp_from_file(const char *path, const pgx_reads *reads, const pgx_db *cdb, pgx_rdp **out)
{
	pgx_db *db = const_cast<pgx_db *>(cdb);
	if (!path || !reads || !db || !out)
		return fail(PGX_E_ARG, "pgx_rdp_from_file: null argument");
	if (!db->bound)
		return fail(PGX_E_ARG, "pgx_rdp_from_file: bind the database to a taxonomy first");
	PGX_TRY(require_device());
	const bool trace = getenv("PGX_TRACE") != nullptr;
	auto t_prev = std::chrono::steady_clock::now();
	const auto t_enter = t_prev;
	// the file's bytes where the page cache holds them (a private read-only mapping: the parsing threads below fault its
	// pages in as they reach them; a copy through read() into a zero-filled string was 0.07 s of a 2 M-line file's 0.55 s);
	// what cannot be mapped (a pipe, an empty file) is read
	struct FileText {
		const char *p = nullptr;
		size_t n = 0;
		void *map = nullptr;
		std::string copy;
		FileText() = default;
		FileText(FileText &&o) : p(o.p), n(o.n), map(o.map), copy(std::move(o.copy)) { o.map = nullptr; }
		~FileText()
		{
			if (map)
				munmap(map, n);
		}
		const char *data() const { return p; }
		size_t size() const { return n; }
		bool empty() const { return n == 0; }
		char back() const { return p[n - 1]; }
	} text;
	{
		const int fd = open(path, O_RDONLY);
		if (fd < 0)
			return fail(PGX_E_IO, "cannot open RDP file %s", path);
		struct stat st;
		if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
			void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
			if (m != MAP_FAILED) {
				text.map = m;
				text.p = (const char *)m;
				text.n = (size_t)st.st_size;
				madvise(m, text.n, MADV_WILLNEED);
			}
		}
		close(fd);
		if (!text.map) {
			bool ok;
			text.copy = read_text_file(path, &ok);
			if (!ok)
				return fail(PGX_E_IO, "cannot open RDP file %s", path);
			text.p = text.copy.data();
			text.n = text.copy.size();
		}
	}
	const size_t n = (size_t)reads->n;
	auto lap = [&](const char *what) {
		if (!trace)
			return;
		const auto now = std::chrono::steady_clock::now();
		fprintf(stderr, "[pgx trace] rdp_from_file %s: %.3f s\n", what, std::chrono::duration<double>(now - t_prev).count());
		t_prev = now;
	};
	lap("file read");
	// The import on the device (rdp_device.hip) whenever the batch's names lie in HBM and do not repeat; the host form below
	// for the rest (synthetic batches, names that repeat, more distinct taxa than the device sets hold) and on request
	// (PGX_RDP_HOST=1: the two forms are compared by the tests)
	if (!getenv("PGX_RDP_HOST")) {
		const int drc = guard("pgx_rdp_from_file", [&]() -> int { return rdp_from_text_device(text.data(), text.size(), reads, db, out); });
		if (drc <= 0) {
			if (trace)
				fprintf(stderr, "[pgx trace] rdp_from_file on the device in all: %.3f s\n",
					std::chrono::duration<double>(std::chrono::steady_clock::now() - t_enter).count());
			return drc;
		}
	}
	// A line belongs to the first read at or after the cursor that carries its name (the streams are in the same
	// order; names may repeat).  The reads are indexed by name hash so that a line of a read that is not in this
	// batch (another shard, another piece of the file) costs one probe, not a walk over the batch.  The passes
	// themselves live in rdp_host.hpp (free of HIP: the build container runs them under the sanitizers).
	ReadNameIndex index(*reads);
	lap("name index");
	int thr = getenv("PGX_RDP_THREADS") ? atoi(getenv("PGX_RDP_THREADS")) : 0; // (measurement aid; clamped: ADVICE r3)
	thr = thr < 0 ? 1 : (thr > 64 ? 64 : thr);
	RdpHostTable ht;
	rdp_parse_host(TextRef{ text.data(), text.size() }, n, index, (unsigned)thr, [&](const std::string &nm) { return db->intern(nm); }, lap, ht);
	std::vector<uint32_t> off(n + 1, 0);
	std::vector<uint32_t> &trips = ht.trips;
	std::vector<uint8_t> &present = ht.present;
	const size_t n_trip = ht.n_trip;
	std::unique_ptr<uint32_t[]> &name_a = ht.name_a, &code_a = ht.code_a;
	std::unique_ptr<int8_t[]> &rank_a = ht.rank_a;
	std::unique_ptr<pgx_rdp> rd(new pgx_rdp());
	rd->n = (int64_t)n;
	rd->max_trip = 0;
	for (size_t r = 0; r < n; r++) {
		off[r + 1] = off[r] + trips[r];
		rd->max_trip = std::max(rd->max_trip, (int)std::min<uint32_t>(trips[r], 8));
	}
	PGX_TRY(rd->d_off.assign(off));
	PGX_TRY(rd->d_name.assign(name_a.get(), n_trip));
	PGX_TRY(rd->d_rank.assign(rank_a.get(), n_trip));
	PGX_TRY(rd->d_code.assign(code_a.get(), n_trip));
	PGX_TRY(rd->d_present.alloc(present.size()));
	PGX_TRY(rd->d_present.upload(present.data(), present.size()));
	lap("offsets, uploads");
	// ~300 MB of work arrays and the file's mapping: unmapping them took 0.02 s of this call's 0.115 s; a thread of its own
	// does it while the caller goes on
	{
		auto junk = std::make_shared<std::tuple<FileText, std::vector<uint32_t>, RdpHostTable, std::vector<uint32_t>, std::vector<uint32_t>, std::vector<uint64_t>>>(
			std::move(text), std::move(off), std::move(ht), std::move(index.slot), std::move(index.next), std::move(index.hash));
		// (a joinable thread, waited for by the next import or at exit: a detached one could still be unmapping when the
		// library is unloaded)
		static std::mutex junk_mu;
		static std::thread junk_thread;
		struct JoinAtExit {
			~JoinAtExit()
			{
				std::lock_guard<std::mutex> lk(junk_mu);
				if (junk_thread.joinable())
					junk_thread.join();
			}
		};
		static JoinAtExit join_at_exit;
		std::lock_guard<std::mutex> lk(junk_mu);
		if (junk_thread.joinable())
			junk_thread.join();
		try {
			junk_thread = std::thread([j = std::move(junk)]() mutable { j.reset(); });
		} catch (...) {
			// (no thread to be had: freed here)
		}
	}
	if (trace)
		fprintf(stderr, "[pgx trace] rdp_from_file in all: %.3f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_enter).count());
	*out = rd.release();
	return 0;
}

// ------------------------------------------------------------------------------------------ three-way vote (opt-in)
// SURVEY 8(f) row 4, spec "pgx-vote3 v1" (restated by the checker in oracle/o_consensus.c): NOT reference behaviour -- the
// reference's Consensus opens the SOAP table and never reads it (Consensus_BLAST_SOAP_RDP-1.1.pl:40-46); this is what
// the tool's name promises.  Per read that has an RDP line, three lineages as (rank 0..6 -> name): B = the read's first
// row of the BLAST table (its best hit), S = the read's first row of the SOAP table, R = the RDP assignment; names are
// the token ids the Consensus comparison uses (same tokeniser, same cleaning).  A rank is agreed when two of the three
// names are equal and not empty (B = S, else B = R, else S = R); the result is the longest prefix of agreed ranks.
static_assert(sizeof(pgx_vote_rec) == 40, "pgx_vote_rec layout");

__global__ void k_vote3(const pgx_hit *__restrict__ hits, const uint32_t *__restrict__ off, const uint32_t *__restrict__ cnt,
			const int32_t *__restrict__ soap_subj, const uint32_t *__restrict__ pairs, uint32_t pair_words, const uint32_t *__restrict__ tok_off,
			const uint32_t *__restrict__ tok, const int8_t *__restrict__ tok_rank, const uint32_t *__restrict__ rdp_off,
			const uint32_t *__restrict__ rdp_code, const uint8_t *__restrict__ rdp_present, uint32_t n,
			pgx_vote_rec *__restrict__ out)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n)
		return;
	uint32_t nm[3][7];
	for (int c = 0; c < 3; c++)
		for (int k = 0; k < 7; k++)
			nm[c][k] = 0u;
	auto lineage_of = [&](int32_t subject, uint32_t (&dst)[7]) { // a rank's name is its FIRST pair, empty or not
		if (subject < 0)
			return;
		uint32_t seen = 0u;
		const uint32_t *rec = pairs + (unsigned long long)pair_words * (uint32_t)subject;
		const uint32_t np = rec[0] >> 16;
		if (np != 0xFFFFu) {
			for (uint32_t a = 0; a < np; a++) {
				const uint32_t pr = rec[1 + a], rk = pr & 7u;
				if (rk >= 1 && !(seen >> rk & 1u)) {
					dst[rk - 1] = pr >> 3;
					seen |= 1u << rk;
				}
			}
		} else { // more pairs than the record holds: the token list
			const uint32_t t0 = tok_off[subject], nt = tok_off[subject + 1] - t0;
			for (uint32_t a = 0; a + 1 < nt; a += 2) {
				const int rk = tok_rank[tok[t0 + a]];
				if (rk >= 0 && !(seen >> (rk + 1) & 1u)) {
					dst[rk] = tok[t0 + a + 1];
					seen |= 1u << (rk + 1);
				}
			}
		}
	};
	lineage_of(cnt[r] ? hits[off[r]].subject : -1, nm[0]);
	lineage_of(soap_subj[r], nm[1]);
	uint32_t seen_r = 0u;
	for (uint32_t t = rdp_off[r]; t < rdp_off[r + 1]; t++) {
		const uint32_t c = rdp_code[t], rk = c & 7u;
		if (c != 0xFFFFFFFFu && rk >= 1 && !(seen_r >> rk & 1u)) {
			nm[2][rk - 1] = c >> 3;
			seen_r |= 1u << rk;
		}
	}
	pgx_vote_rec v;
	v.depth = rdp_present[r] ? 0 : -1; // -1: the read has no RDP line (no line of text either)
	for (int k = 0; k < 7; k++) {
		v.name[k] = 0u;
		v.votes[k] = 0;
	}
	v.pad = 0;
	if (v.depth == 0) {
		for (int k = 0; k < 7; k++) {
			const uint32_t b = nm[0][k], s = nm[1][k], q = nm[2][k];
			uint32_t w = 0u, votes = 0u;
			if (b && b == s) {
				w = b;
				votes = 2u + (q == b ? 1u : 0u);
			} else if (b && b == q) {
				w = b;
				votes = 2u;
			} else if (s && s == q) {
				w = s;
				votes = 2u;
			}
			if (!votes)
				break;
			v.name[k] = w;
			v.votes[k] = (uint8_t)votes;
			v.depth = k + 1;
		}
	}
	out[r] = v;
}

extern "C" int pgx_vote3_batch(const pgx_db *db, const pgx_reads *reads, const pgx_hits *hits, const pgx_rdp *rdp, const char *soap_path,
			       pgx_vote_rec *out, int64_t cap)
{
	if (!db || !reads || !hits || !rdp || !soap_path || !out)
		return fail(PGX_E_ARG, "pgx_vote3_batch: null argument");
	if (!db->bound)
		return fail(PGX_E_ARG, "pgx_vote3_batch: bind the database to a taxonomy first");
	if (hits->n_reads != reads->n || rdp->n != reads->n || cap < reads->n)
		return fail(PGX_E_ARG, "pgx_vote3_batch: the tables cover different read counts");
	PGX_TRY(require_device());
	return pgx::guard("pgx_vote3_batch", [&]() -> int {
		bool ok;
		const std::string text = read_text_file(soap_path, &ok);
		if (!ok)
			return fail(PGX_E_IO, "Error: Unable to open %s file.", soap_path);
		const size_t n = (size_t)reads->n;
		// SOAP rows (soap.man: column 1 read name, column 8 reference id): the first row of every read
		std::vector<int32_t> subj(n ? n : 1, -1);
		std::unordered_map<std::string, uint32_t> id_of;
		id_of.reserve((size_t)db->n_seq * 2);
		for (size_t i = 0; i < (size_t)db->n_seq; i++)
			id_of.emplace(db->ids[i], (uint32_t)i);
		const ReadNameIndex index(*reads);
		for (size_t s0 = 0; s0 < text.size();) {
			const char *nl = (const char *)memchr(text.data() + s0, '\n', text.size() - s0);
			const size_t e = nl ? (size_t)(nl - text.data()) : text.size();
			const char *line = text.data() + s0;
			const size_t len = e - s0;
			s0 = e + 1;
			const char *tab = (const char *)memchr(line, '\t', len);
			if (!tab)
				continue;
			const size_t r = index.find(line, (size_t)(tab - line), 0);
			if (r >= n || subj[r] != -1)
				continue;
			const char *p = tab + 1;
			for (int col = 1; col < 7 && p; col++) {
				const char *t2 = (const char *)memchr(p, '\t', (size_t)(line + len - p));
				p = t2 ? t2 + 1 : nullptr;
			}
			if (!p)
				continue;
			const char *t2 = (const char *)memchr(p, '\t', (size_t)(line + len - p));
			auto it = id_of.find(std::string(p, t2 ? (size_t)(t2 - p) : (size_t)(line + len - p)));
			subj[r] = it == id_of.end() ? -2 : (int32_t)it->second; // -2: a reference the database does not hold (no vote)
		}
		for (auto &x : subj)
			if (x == -2)
				x = -1;
		DevBuf<int32_t> d_subj;
		DevBuf<pgx_vote_rec> d_out;
		PGX_TRY(d_subj.alloc(n ? n : 1));
		PGX_TRY(d_subj.upload(subj.data(), n));
		PGX_TRY(d_out.alloc(n ? n : 1));
		if (n) {
			hipLaunchKernelGGL(k_vote3, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, 0, hits->d_hits.data(), hits->d_read_off.data(),
					   hits->d_read_cnt.data(), d_subj.data(), db->d_subj_pairs.data(), (uint32_t)db->pair_words, db->d_subj_tok_off.data(),
					   db->d_subj_tok.data(), db->d_tok_rank.data(), rdp->d_off.data(), rdp->d_code.data(), rdp->d_present.data(),
					   (uint32_t)n, d_out.data());
			PGX_HIP(hipGetLastError());
			PGX_TRY(d_out.download(out, n));
		}
		return 0;
	});
}

extern "C" int pgx_vote3_format(const pgx_db *db, const pgx_reads *reads, const pgx_vote_rec *recs, int64_t n, char **text, size_t *len)
{
	if (!db || !reads || !recs || !text)
		return fail(PGX_E_ARG, "pgx_vote3_format: null argument");
	return pgx::guard("pgx_vote3_format", [&]() -> int {
		Text out;
		for (int64_t r = 0; r < n && r < reads->n; r++) {
			const pgx_vote_rec &v = recs[r];
			if (v.depth < 0)
				continue;
			out.s += reads->name_of(r);
			out.s += '\t';
			std::string votes;
			for (int k = 0; k < v.depth && k < 7; k++) {
				out.printf("[%d]", k);
				out.s += v.name[k] < db->token_text.size() ? db->token_text[v.name[k]] : std::string();
				out.s += ';';
				votes += (char)('0' + v.votes[k]);
			}
			out.printf("\t%d\t%s\n", v.depth, votes.c_str());
		}
		*text = out.release_malloc(len);
		return *text ? 0 : fail(PGX_E_NOMEM, "out of memory");
	});
}

static void synth_level_counts(const pgx_synth_cfg *c, int64_t cnt[7], int64_t base[7])
{
	auto max1 = [](int64_t v) { return v < 1 ? (int64_t)1 : v; };
	cnt[6] = c->n_seq;
	cnt[5] = c->n_genus;
	cnt[4] = max1(cnt[5] / 5);
	cnt[3] = max1(cnt[4] / 4);
	cnt[2] = max1(cnt[3] / 5);
	cnt[1] = max1(cnt[2] / 5);
	cnt[0] = max1(cnt[1] / 20);
	int64_t b = 2;
	for (int l = 0; l < 7; l++) {
		base[l] = b;
		b += cnt[l];
	}
}

int pgx_rdp_from_synth(const pgx_synth_cfg *cfg, int64_t first, int64_t count, const pgx_db *db, pgx_rdp **out)
{
	if (!cfg || !db || !out || count < 0)
		return fail(PGX_E_ARG, "pgx_rdp_from_synth: bad argument");
	if (!db->bound)
		return fail(PGX_E_ARG, "pgx_rdp_from_synth: bind the database to the synthetic taxonomy first");
	PGX_TRY(require_device());
	int64_t cnt[7], base[7];
	synth_level_counts(cfg, cnt, base);
	if ((size_t)(base[6] + cnt[6]) > db->d_node_name_tok.n)
		return fail(PGX_E_ARG, "bound taxonomy is smaller than the synthetic one");
	DevBuf<int64_t> d_cnt, d_base;
	PGX_TRY(d_cnt.assign(cnt, 7));
	PGX_TRY(d_base.assign(base, 7));
	std::unique_ptr<pgx_rdp> rd(new pgx_rdp());
	rd->n = count;
	rd->max_trip = 6; // the synthetic stream names six ranks per read
	std::vector<uint32_t> off((size_t)count + 1);
	for (int64_t i = 0; i <= count; i++)
		off[(size_t)i] = (uint32_t)(6 * i);
	PGX_TRY(rd->d_off.assign(off));
	PGX_TRY(rd->d_name.alloc((size_t)count * 6 + 1));
	PGX_TRY(rd->d_rank.alloc((size_t)count * 6 + 1));
	PGX_TRY(rd->d_code.alloc((size_t)count * 6 + 1));
	PGX_TRY(rd->d_present.alloc((size_t)count + 1));
	if (hipMemset(rd->d_present.data(), 1, (size_t)count + 1) != hipSuccess)
		return fail(PGX_E_NODEVICE, "hipMemset failed");
	if (count > 0) {
		hipLaunchKernelGGL(k_synth_rdp, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, cfg->read_seed,
				   (uint64_t)cfg->n_seq, (uint32_t)cfg->seq_len, (uint32_t)cfg->read_len, (uint64_t)first,
				   (uint64_t)count, d_cnt.data(), d_base.data(), db->d_node_name_tok.data(), rd->d_name.data(),
				   rd->d_rank.data(), rd->d_code.data());
		if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
			return fail(PGX_E_NODEVICE, "k_synth_rdp failed");
	}
	index_check(db, "rdp_from_synth");
	*out = rd.release();
	return 0;
}

int pgx_synth_write_taxdump(const pgx_synth_cfg *c, const char *dir)
{
	if (!c || !dir)
		return fail(PGX_E_ARG, "pgx_synth_write_taxdump: null argument");
	static const char *const rank_name[7] = { "superkingdom", "phylum", "class", "order", "family", "genus", "species" };
	static const char *const prefix[6] = { "Dom", "Phy", "Cls", "Ord", "Fam", "Gen" };
	int64_t cnt[7], base[7];
	synth_level_counts(c, cnt, base);
	std::string d = dir;
	FILE *fn = fopen((d + "/nodes.dmp").c_str(), "w");
	FILE *fm = fopen((d + "/names.dmp").c_str(), "w");
	FILE *fg = fopen((d + "/gi_taxid_nucl.dmp").c_str(), "w");
	if (!fn || !fm || !fg) {
		if (fn) fclose(fn);
		if (fm) fclose(fm);
		if (fg) fclose(fg);
		return fail(PGX_E_IO, "cannot write taxonomy dumps into %s", dir);
	}
	auto alpha5 = [](int64_t k, char *o) {
		for (int p = 4; p >= 0; p--) {
			o[p] = (char)('a' + k % 26);
			k /= 26;
		}
		o[5] = 0;
	};
	fprintf(fn, "1\t|\t1\t|\tno rank\t|\t\t|\t8\t|\t0\t|\t1\t|\t0\t|\t0\t|\t0\t|\t0\t|\t0\t|\t\t|\n");
	fprintf(fm, "1\t|\troot\t|\t\t|\tscientific name\t|\n");
	char a[8], g[8];
	for (int l = 0; l < 7; l++)
		for (int64_t k = 0; k < cnt[l]; k++) {
			const int64_t id = base[l] + k;
			const int64_t par = l == 0 ? 1 : base[l - 1] + (int64_t)(((unsigned __int128)k * (uint64_t)cnt[l - 1]) / (uint64_t)cnt[l]);
			fprintf(fn, "%lld\t|\t%lld\t|\t%s\t|\t\t|\t0\t|\t1\t|\t11\t|\t1\t|\t0\t|\t1\t|\t0\t|\t0\t|\t\t|\n",
				(long long)id, (long long)par, rank_name[l]);
			alpha5(k, a);
			if (l < 6) {
				fprintf(fm, "%lld\t|\t%s%s\t|\t\t|\tscientific name\t|\n", (long long)id, prefix[l], a);
			} else {
				alpha5((int64_t)(((unsigned __int128)k * (uint64_t)cnt[5]) / (uint64_t)cnt[6]), g);
				fprintf(fm, "%lld\t|\tGen%s sp%s\t|\t\t|\tscientific name\t|\n", (long long)id, g, a);
			}
		}
	// `tax_class -n` never finds the last record of names.dmp (ncbitc.c:665): keep it a dummy
	fprintf(fm, "%lld\t|\tzz sentinel\t|\t\t|\tsynonym\t|\n", (long long)(base[6] + cnt[6] - 1));
	for (int64_t i = 0; i < c->n_seq; i++)
		fprintf(fg, "%lld\t%lld\n", (long long)(1000 + i), (long long)(base[6] + i));
	fclose(fn);
	fclose(fm);
	fclose(fg);
	return 0;
}

int pgx_consensus_format(const pgx_db *db, const pgx_reads *reads, const pgx_hits *hits, const pgx_consensus_rec *recs,
			 int64_t n, char **text, size_t *len)
{
	if (!db || !reads || !hits || !recs || !text)
		return fail(PGX_E_ARG, "pgx_consensus_format: null argument");
	if (!db->bound)
		return fail(PGX_E_ARG, "pgx_consensus_format: database is not bound to a taxonomy");
	if (n > reads->n)
		n = reads->n;
	{
		// rendered by kernels (blast_format.hip); the host loop below serves batches of long, all-different queries
		Text dev;
		int drc = 0;
		if (consensus_format_device(db, reads, hits, recs, n, dev.s, &drc)) {
			PGX_TRY(drc);
			*text = dev.release_malloc(len);
			return *text ? 0 : fail(PGX_E_NOMEM, "out of memory");
		}
	}
	std::vector<pgx_hit> hv((size_t)hits->n_hits);
	PGX_TRY(hits->d_hits.download(hv.data(), hv.size()));
	Text out;
	Text cols;
	for (int64_t r = 0; r < n && r < reads->n; r++) {
		if (recs[r].hit == -2)
			continue; // no BLAST lines for this read: the Perl prints nothing for it
		if (recs[r].hit >= 0) {
			const pgx_hit &h = hv[(size_t)recs[r].hit];
			// the line NCBI-taxcollector writes for this hit: id, lineage, then the numeric columns
			// with the blank in front of a 3-digit bit score eaten by its split (taxcollector:77,148-153)
			std::string line = reads->name_of(r) + "\t" + db->ids[(size_t)h.subject] + "\t";
			cols.s.clear();
			format_hit_columns(h, reads->h_len[(size_t)r], db->n_bases, db->n_seq, hits->gapped, cols);
			line += cols.s;
			emit_collected(line, db->lineage[(size_t)h.subject], out.s);
		} else {
			out.s += "\n";
		}
		out.printf("#Matches found: %d\n", recs[r].matches);
	}
	*text = out.release_malloc(len);
	return *text ? 0 : fail(PGX_E_NOMEM, "out of memory");
}

// The same text straight into a file (`-o` of the Consensus script, Consensus_BLAST_SOAP_RDP-1.1.pl:52): rendered on the
// device in pieces of 256 k reads; a piece is written while the next one is rendered and copied into the other of two
// pinned buffers.  (Through pgx_consensus_format the 319 MB of a 2 M-read batch went through four host copies: 0.28 s.)
int pgx_consensus_format_file(const pgx_db *db, const pgx_reads *reads, const pgx_hits *hits, const pgx_consensus_rec *recs,
			      int64_t n, const char *path, size_t *bytes_out)
{
	if (!db || !reads || !hits || !recs || !path)
		return fail(PGX_E_ARG, "pgx_consensus_format_file: null argument");
	if (!db->bound)
		return fail(PGX_E_ARG, "pgx_consensus_format_file: database is not bound to a taxonomy");
	if (n > reads->n)
		n = reads->n;
	// The text goes to a file beside `path` and takes its name when all of it is written: a render that fails no longer leaves
	// the caller's file truncated.  What is not a regular file (a pipe, /dev/stdout) is written in place.
	struct stat st;
	const bool in_place = stat(path, &st) == 0 && !S_ISREG(st.st_mode);
	const std::string tmp_path = in_place ? std::string(path) : std::string(path) + ".part" + std::to_string((long long)getpid());
	FILE *f = fopen(tmp_path.c_str(), "wb");
	if (!f)
		return fail(PGX_E_IO, "Unable to open %s", path);
	size_t total = 0;
	int drc = 0;
	bool io_ok = true;
	const bool on_device = consensus_format_pieces(db, reads, hits, recs, n, 256u << 10, [&](const char *p, size_t b) {
		if (fwrite(p, 1, b, f) != b)
			io_ok = false;
		total += b;
		return 0;
	}, &drc);
	int rc = drc;
	if (!on_device) { // (batches of long, all-different queries: the host rendering)
		char *text = nullptr;
		size_t len = 0;
		rc = pgx_consensus_format(db, reads, hits, recs, n, &text, &len);
		if (rc >= 0) {
			io_ok = fwrite(text, 1, len, f) == len;
			total = len;
		}
		free(text);
	}
	if (fclose(f) != 0)
		io_ok = false;
	if (!in_place) {
		if (rc < 0 || !io_ok)
			unlink(tmp_path.c_str());
		else if (rename(tmp_path.c_str(), path) != 0) {
			unlink(tmp_path.c_str());
			io_ok = false;
		}
	}
	if (rc < 0)
		return rc;
	if (!io_ok)
		return fail(PGX_E_IO, "write to %s failed", path);
	if (bytes_out)
		*bytes_out = total;
	return 0;
}

int pgx_consensus_batch(const pgx_db *db, const pgx_hits *hits, const pgx_rdp *rdp, pgx_consensus_rec *out, int64_t cap)
{
	if (!db || !hits || !rdp || !out || cap < hits->n_reads)
		return fail(PGX_E_ARG, "pgx_consensus_batch: bad argument");
	PGX_TRY(require_device());
	DevBuf<pgx_consensus_rec> d_recs;
	PGX_TRY(d_recs.alloc((size_t)hits->n_reads + 1));
	PGX_TRY(consensus_device(db, hits, rdp, d_recs.data(), nullptr));
	return d_recs.download(out, (size_t)hits->n_reads);
}

int pgx_consensus_file(const char *b, const char *r, const char *s_or_null, const char *o, char **log_text)
{
	Text log;
	return with_text(log, log_text, [&]() -> int {
		if (!b || !r || !o)
			return fail(PGX_E_ARG, "consensus: -b, -r and -o are required");
		PGX_TRY(require_device());
		log.s += "\nLoading input files...\n"; // Consensus:19
		const bool trace = getenv("PGX_TRACE") != nullptr;
		auto t_now = [] { return std::chrono::steady_clock::now(); };
		auto t_ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
			return std::chrono::duration<double, std::milli>(b - a).count();
		};
		const auto t0 = t_now();
		bool ok;
		std::string bt = read_text_file(b, &ok);
		if (!ok) {
			log.printf("Error: Unable to open %s file.\n", b);
			return fail(PGX_E_IO, "cannot open %s", b);
		}
		std::string rt = read_text_file(r, &ok);
		if (!ok) {
			log.printf("Error: Unable to open %s file.\n", r);
			return fail(PGX_E_IO, "cannot open %s", r);
		}
		if (s_or_null && *s_or_null) {
			FILE *f = fopen(s_or_null, "r"); // opened and never read (Consensus:40-46)
			if (!f) {
				log.printf("Error: Unable to open %s file.\n", s_or_null);
				return fail(PGX_E_IO, "cannot open %s", s_or_null);
			}
			fclose(f);
		}
		log.printf("%s\n", o); // Consensus:51

		const auto t1 = t_now();
		// ---- BLAST(+lineage) table: id, lineage tokens, similarity text per line (Consensus:110-122)
		std::unordered_map<std::string, uint32_t> tmap;
		std::vector<std::string> ttext;
		intern_into(tmap, ttext, "");
		// Nothing is copied per line: lines and their id are spans of the file text.  Pass A (all host cores, contiguous
		// pieces of the file): line boundaries, the first three columns of split(/\t\t|\t/) and a 64-bit hash of the
		// lineage and similarity texts.  Pass B (one thread): the lineage column is tokenised once per DISTINCT text (a
		// hit table names a few hundred thousand lineages millions of times) and the similarity column ranked once per
		// distinct text; equal hashes are confirmed by comparing the texts.
		struct Span {
			size_t s, n;
		};
		struct LineInfo {
			size_t s;
			uint32_t n, id_n, lin_s, lin_n, sim_s, sim_n; // column offsets are relative to the line start
			uint64_t lin_h, sim_h;
		};
		auto fnv64 = [](const char *p, size_t n) {
			uint64_t h = 1469598103934665603ull;
			for (size_t i = 0; i < n; i++)
				h = (h ^ (unsigned char)p[i]) * 1099511628211ull;
			return h;
		};
		const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
		const unsigned workers = (unsigned)std::max<size_t>(1, std::min<size_t>(hw, bt.size() / (4u << 20) + 1));
		std::vector<std::vector<LineInfo>> part(workers);
		{
			// piece w = [cut[w], cut[w+1]) where every cut is a line start
			std::vector<size_t> cut(workers + 1, bt.size());
			cut[0] = 0;
			for (unsigned w = 1; w < workers; w++) {
				size_t c = bt.size() * w / workers;
				const char *nl = c < bt.size() ? (const char *)memchr(bt.data() + c, '\n', bt.size() - c) : nullptr;
				cut[w] = nl ? (size_t)(nl - bt.data()) + 1 : bt.size();
			}
			auto scan = [&](unsigned w) {
				std::vector<LineInfo> &out = part[w];
				out.reserve((cut[w + 1] - cut[w]) / 60 + 16);
				for (size_t s = cut[w]; s < cut[w + 1];) {
					const char *nl = (const char *)memchr(bt.data() + s, '\n', bt.size() - s);
					const size_t e = nl ? (size_t)(nl - bt.data()) : bt.size();
					const char *ln = bt.data() + s;
					const size_t n = e - s;
					// split(/\t\t|\t/): fields 0, 1, 2 in place (a trailing empty field does not exist)
					Span f[3] = { { 0, 0 }, { 0, 0 }, { 0, 0 } };
					int nf = 0;
					size_t a = 0, i = 0;
					while (i < n && nf < 3) {
						if (ln[i] == '\t') {
							f[nf++] = { a, i - a };
							i += (i + 1 < n && ln[i + 1] == '\t') ? 2 : 1;
							a = i;
						} else {
							i++;
						}
					}
					if (nf < 3 && n > 0 && a < n)
						f[nf++] = { a, n - a };
					LineInfo li;
					li.s = s;
					li.n = (uint32_t)n;
					li.id_n = (uint32_t)f[0].n;
					li.lin_s = (uint32_t)f[1].s;
					li.lin_n = (uint32_t)f[1].n;
					li.sim_s = (uint32_t)f[2].s;
					li.sim_n = (uint32_t)f[2].n;
					li.lin_h = fnv64(ln + f[1].s, f[1].n);
					li.sim_h = fnv64(ln + f[2].s, f[2].n);
					out.push_back(li);
					s = e + 1;
				}
			};
			if (workers == 1) {
				scan(0);
			} else {
				std::vector<std::thread> th;
				for (unsigned w = 0; w < workers; w++)
					th.emplace_back(scan, w);
				for (auto &t : th)
					t.join();
			}
		}
		size_t n_lines = 0;
		for (auto &v : part)
			n_lines += v.size();
		std::vector<Span> bline, bid;
		bline.reserve(n_lines);
		bid.reserve(n_lines);
		std::vector<uint32_t> tok_off(1, 0), tok;
		tok.reserve(n_lines * 14);
		std::vector<std::string> tk;
		struct Memo {
			size_t s;
			uint32_t n, first, count; // representative text (file offset, length), its tokens in lin_tok
		};
		std::unordered_multimap<uint64_t, Memo> lin_memo;
		std::vector<uint32_t> lin_tok;
		struct SimMemo {
			size_t s;
			uint32_t n, id;
		};
		std::unordered_multimap<uint64_t, SimMemo> sim_memo;
		std::vector<std::string> sim_text;
		std::vector<uint32_t> line_simid;
		line_simid.reserve(n_lines);
		for (auto &v : part) {
			for (const LineInfo &li : v) {
				bline.push_back({ li.s, li.n });
				bid.push_back({ li.s, li.id_n });
				const char *simp = bt.data() + li.s + li.sim_s, *linp = bt.data() + li.s + li.lin_s;
				uint32_t sid = 0xFFFFFFFFu;
				for (auto r = sim_memo.equal_range(li.sim_h); r.first != r.second; ++r.first)
					if (r.first->second.n == li.sim_n && memcmp(bt.data() + r.first->second.s, simp, li.sim_n) == 0) {
						sid = r.first->second.id;
						break;
					}
				if (sid == 0xFFFFFFFFu) {
					sid = (uint32_t)sim_text.size();
					sim_text.emplace_back(simp, li.sim_n);
					sim_memo.emplace(li.sim_h, SimMemo{ li.s + li.sim_s, li.sim_n, sid });
				}
				line_simid.push_back(sid);
				const Memo *m = nullptr;
				for (auto r = lin_memo.equal_range(li.lin_h); r.first != r.second; ++r.first)
					if (r.first->second.n == li.lin_n && memcmp(bt.data() + r.first->second.s, linp, li.lin_n) == 0) {
						m = &r.first->second;
						break;
					}
				if (!m) {
					lineage_tokens(std::string(linp, li.lin_n), tk);
					const uint32_t t0 = (uint32_t)lin_tok.size();
					for (auto &t : tk)
						lin_tok.push_back(intern_into(tmap, ttext, t));
					m = &lin_memo.emplace(li.lin_h, Memo{ li.s + li.lin_s, li.lin_n, t0, (uint32_t)tk.size() })->second;
				}
				tok.insert(tok.end(), lin_tok.begin() + m->first, lin_tok.begin() + m->first + m->count);
				tok_off.push_back((uint32_t)tok.size());
			}
			std::vector<LineInfo>().swap(v);
		}
		std::map<std::string, uint32_t> simrank;
		build_sim_ranks(sim_text, simrank);
		std::vector<uint32_t> simid_rank(sim_text.size());
		for (size_t i = 0; i < sim_text.size(); i++)
			simid_rank[i] = simrank[sim_text[i]];
		std::vector<uint32_t> line_sim(bline.size());
		for (size_t i = 0; i < bline.size(); i++)
			line_sim[i] = simid_rank[line_simid[i]];
		auto id_equals = [&](size_t line, const std::string &x) {
			return bid[line].n == x.size() && memcmp(bt.data() + bid[line].s, x.data(), x.size()) == 0;
		};

		const auto t2 = t_now();
		// ---- RDP lines (Consensus:126-132) and the cursor walk over both files (Consensus:96-240)
		std::vector<uint32_t> rdp_off(1, 0), rdp_name;
		std::vector<int8_t> rdp_rank;
		std::vector<uint32_t> g_first, g_count, g_rdp, g_init;
		size_t cur = 0;
		int found = -1; // undef
		bool sim_is_undef = true;
		int status = 0;
		uint32_t rdp_index = 0;
		for (size_t s = 0; s < rt.size() && status == 0;) {
			size_t e = rt.find('\n', s);
			if (e == std::string::npos)
				e = rt.size();
			std::string line(rt, s, e - s);
			s = e + 1;
			size_t five = line.find("\t\t\t\t\t");
			std::string rid = five == std::string::npos ? line : line.substr(0, five);
			if (five != std::string::npos) {
				std::string rest = line.substr(five + 5);
				size_t again = rest.find("\t\t\t\t\t");
				if (again != std::string::npos)
					rest.resize(again);
				std::vector<std::string> f;
				if (!rest.empty()) {
					for (size_t a = 0; a <= rest.size();) {
						size_t t = rest.find('\t', a);
						if (t == std::string::npos)
							t = rest.size();
						f.emplace_back(rest, a, t - a);
						a = t + 1;
					}
				}
				while (!f.empty() && f.back().empty())
					f.pop_back();
				for (size_t k = 0; k < f.size(); k += 3) {
					rdp_name.push_back(intern_into(tmap, ttext, clean_rdp_name(f[k])));
					rdp_rank.push_back(k + 1 < f.size() ? rdp_rank_index(f[k + 1]) : (int8_t)-1);
				}
			}
			rdp_off.push_back((uint32_t)rdp_name.size());
			// GETBLAST loop
			uint32_t first = (uint32_t)cur, count = 0;
			for (;;) {
				const bool have = cur < bline.size();
				if (have ? id_equals(cur, rid) : rid.empty()) {
					if (!have) {
						status = fail(PGX_E_REFHANG, "RDP line %u has an empty id after the BLAST table ends: the reference never terminates", rdp_index + 1);
						break;
					}
					if (count == 0)
						first = (uint32_t)cur;
					found = 1;
					count++;
					cur++;
					continue;
				}
				if (found == 0) {
					const std::string id = have ? std::string(bt, bid[cur].s, bid[cur].n) : std::string();
					log.printf("not found: %s\t %s\n", id.c_str(), rid.c_str()); // Consensus:217
					if (!have) {
						status = fail(PGX_E_REFHANG, "RDP read %s has no BLAST lines at or after the cursor: the reference never terminates (SURVEY 3.5)", rid.c_str());
						break;
					}
					cur++;
					continue;
				}
				if (found == 1) {
					g_first.push_back(first);
					g_count.push_back(count);
					g_rdp.push_back(rdp_index);
					g_init.push_back(sim_is_undef ? simrank[""] : simrank["0"]);
					sim_is_undef = false;
					found = 0;
				}
				break;
			}
			rdp_index++;
		}

		const auto t3 = t_now();
		// ---- device: agreement counts + arg-max per group
		const size_t ng = g_first.size();
		std::vector<pgx_consensus_rec> recs(ng);
		if (ng) {
			std::vector<int8_t> tok_rank(ttext.size());
			for (size_t t = 0; t < ttext.size(); t++)
				tok_rank[t] = blast_rank_index(ttext[t]);
			DevBuf<uint32_t> d_first, d_count, d_grdp, d_init, d_toff, d_tok, d_sim, d_roff, d_rname;
			DevBuf<int8_t> d_trank, d_rrank;
			DevBuf<pgx_consensus_rec> d_recs;
			PGX_TRY(d_first.assign(g_first));
			PGX_TRY(d_count.assign(g_count));
			PGX_TRY(d_grdp.assign(g_rdp));
			PGX_TRY(d_init.assign(g_init));
			PGX_TRY(d_toff.assign(tok_off));
			PGX_TRY(d_tok.assign(tok));
			PGX_TRY(d_sim.assign(line_sim));
			PGX_TRY(d_roff.assign(rdp_off));
			PGX_TRY(d_rname.assign(rdp_name));
			PGX_TRY(d_trank.assign(tok_rank));
			PGX_TRY(d_rrank.assign(rdp_rank));
			PGX_TRY(d_recs.alloc(ng));
			hipLaunchKernelGGL(k_consensus_groups, dim3((unsigned)((ng + 63) / 64)), dim3(64), 0, 0, d_first.data(),
					   d_count.data(), d_grdp.data(), d_init.data(), (uint32_t)ng, d_toff.data(), d_tok.data(),
					   d_trank.data(), d_sim.data(), d_roff.data(), d_rname.data(), d_rrank.data(), d_recs.data());
			if (hipGetLastError() != hipSuccess)
				return fail(PGX_E_NODEVICE, "k_consensus_groups launch failed");
			PGX_TRY(d_recs.download(recs.data(), ng));
		}
		std::string out;
		for (size_t g = 0; g < ng; g++) {
			if (recs[g].hit >= 0)
				out.append(bt, bline[(size_t)recs[g].hit].s, bline[(size_t)recs[g].hit].n);
			out += "\n";
			char tmp[64];
			snprintf(tmp, sizeof tmp, "#Matches found: %d\n", recs[g].matches);
			out += tmp;
		}
		const auto t4 = t_now();
		int wrc = write_text_file(o, out);
		if (wrc < 0) {
			log.printf("Error: Unable to open output file %s.\n", o);
			return wrc;
		}
		if (trace)
			fprintf(stderr, "[pgx trace] consensus verb: files %.0f ms, hit table %.0f ms, RDP + cursor walk %.0f ms, device + text %.0f ms, write %.0f ms\n",
				t_ms(t0, t1), t_ms(t1, t2), t_ms(t2, t3), t_ms(t3, t4), t_ms(t4, t_now()));
		if (status == 0)
			log.s += "\nDone!\n"; // Consensus:242
		return status;
	});
}
}
