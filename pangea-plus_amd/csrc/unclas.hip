// Unclas_Sel/unclassified_selector.pl: the reads Classify left without a row that passes the three
// thresholds, for a second search with looser settings or against another database.
//
//   pgx_unclas_file          the reference command line on a table and a FASTA file: the host splits lines, cuts and numifies
//                            the columns (the script's own index / rindex / substr arithmetic) and interns the names; row
//                            flags, the OR per name, the first header of a name and the fate of every FASTA line are
//                            computed on the device
//   pgx_unclassified_batch   the same selection straight from the hit table and the read batch in HBM: one pass over the
//                            slot table with integer thresholds, then the selected reads' packed bases unpacked into the
//                            records of a DeviceFasta, which the import's second half turns into a batch
#include <rocprim/device/device_scan.hpp>

#include <cerrno>
#include <cmath>
#include <cstring>

#include "engine.hpp"
#include "perlops.hpp"

namespace pgx {

constexpr uint32_t kNotHeader = 0xFFFFFFFEu; // FASTA line that is no header
constexpr uint32_t kNoName = 0xFFFFFFFFu;    // header whose name no table row carries

// ------------------------------------------------------------------------------------------ file form: device part
// a name is classified when one of its rows passes (unclassified_selector.pl:96-110); racing stores write the same byte
__global__ void k_un_name_or(const uint8_t *__restrict__ pass, const uint32_t *__restrict__ row_name, uint64_t n,
			     uint8_t *__restrict__ classified)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n && pass[i])
		classified[row_name[i]] = 1;
}

// the script deletes a classified name at its first header (:143-153): only that header is dropped
__global__ void k_un_first_header(const uint32_t *__restrict__ hdr_name, uint32_t n_lines, uint32_t *__restrict__ first)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_lines)
		return;
	const uint32_t k = hdr_name[i];
	if (k < kNotHeader)
		atomicMin(&first[k], i);
}

// per FASTA line: 0, or for a header (line + 1) << 1 | printed; the running maximum of these carries a header's fate to
// the lines behind it (:162-165)
__global__ void k_un_line_fate(const uint32_t *__restrict__ hdr_name, const uint8_t *__restrict__ classified,
			       const uint32_t *__restrict__ first, uint32_t n_lines, uint32_t *__restrict__ fate)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_lines)
		return;
	const uint32_t k = hdr_name[i];
	uint32_t f = 0;
	if (k != kNotHeader) {
		const bool dropped = k != kNoName && classified[k] && first[k] == i;
		f = ((i + 1) << 1) | (dropped ? 0u : 1u);
	}
	fate[i] = f;
}

// ------------------------------------------------------------------------------------------ resident form: device part
// One lane per slot of the hit table, whole 32-byte records as two 16-byte loads.  Only the first read_cnt[read] slots of
// a read are rows of the text (the ones behind hold S3c duplicates and subjects past the 500th); a passing row marks its
// read with a plain byte store (every racing lane stores the same 1).
__global__ __launch_bounds__(256) void k_un_rows(const pgx_hit *__restrict__ hits, uint64_t n_slots, const uint32_t *__restrict__ read_off,
						 const uint32_t *__restrict__ read_cnt, const uint32_t *__restrict__ read_len, uint32_t n_reads,
						 int h_min, const uint32_t *__restrict__ s_min, uint32_t max_len, uint8_t *__restrict__ classified)
{
	const uint4 *rec = reinterpret_cast<const uint4 *>(hits);
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_slots; i += (uint64_t)gridDim.x * 256) {
		const uint4 a = rec[2 * i], b = rec[2 * i + 1];
		pgx_hit h;
		h.read = (int32_t)a.x;
		h.subject = (int32_t)a.y;
		h.qstart = (int32_t)a.z;
		h.qend = (int32_t)a.w;
		h.sstart = (int32_t)b.x;
		h.send = (int32_t)b.y;
		h.score = (int32_t)b.z;
		h.mismatch = (uint16_t)(b.w & 0xFFFFu);
		h.gapopen = (uint16_t)(b.w >> 16);
		const uint32_t r = (uint32_t)h.read;
		if (r >= n_reads)
			continue;
		const uint32_t off = read_off[r];
		if (i < off || i - off >= read_cnt[r])
			continue;
		const int len = hit_length(h);
		if (len <= 0)
			continue;
		const int hund = pident_hundredths(len - hit_diffs(h), len);
		const uint32_t L = read_len[r];
		const uint32_t smin = L <= max_len ? s_min[L] : 0xFFFFFFFFu;
		if (hund >= h_min && h.score >= 0 && (uint32_t)h.score >= smin)
			classified[r] = 1;
	}
}

// duplicate read names: a name is classified when one of its reads is, and its first read is the one dropped
__global__ void k_un_group(const uint8_t *__restrict__ classified, const uint32_t *__restrict__ gid, uint32_t n,
			   uint8_t *__restrict__ g_classified, uint32_t *__restrict__ g_first)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n)
		return;
	const uint32_t g = gid[r];
	if (classified[r])
		g_classified[g] = 1;
	atomicMin(&g_first[g], r);
}

// The mask, and per read (n + 1 entries, the last one 0) what a selected read adds to the subset batch: one record, its
// letters, its name bytes.  gid null: names are unique, the mask is !classified.
__global__ void k_un_mask(const uint8_t *__restrict__ classified, const uint32_t *__restrict__ gid, const uint8_t *__restrict__ g_classified,
			  const uint32_t *__restrict__ g_first, const uint32_t *__restrict__ read_len, const uint32_t *__restrict__ name_at,
			  unsigned long long first_ordinal, uint32_t n, uint8_t *__restrict__ mask, uint32_t *__restrict__ add_rec,
			  uint64_t *__restrict__ add_let, uint64_t *__restrict__ add_name)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r > n)
		return;
	uint32_t m = 0, nb = 0, L = 0;
	if (r < n) {
		if (gid) {
			const uint32_t g = gid[r];
			m = !(g_classified[g] && g_first[g] == r);
		} else {
			m = !classified[r];
		}
		mask[r] = (uint8_t)m;
		if (m) {
			L = read_len[r];
			if (name_at) {
				nb = name_at[r + 1] - name_at[r];
			} else { // synthetic batch: "r<first + r>"
				nb = 2;
				for (unsigned long long v = (first_ordinal + r) / 10; v; v /= 10)
					nb++;
			}
		}
	}
	add_rec[r] = m;
	add_let[r] = L;
	add_name[r] = nb;
}

constexpr int kUnGroup = 32; // lanes that unpack one read

// The selected reads as records of a DeviceFasta: letters A/C/G/T (N where the ambiguity word says so) from the packed
// forward strand, names from the batch's own name bytes, offsets per record.  kUnGroup lanes per read of the SOURCE batch
// (the scans are indexed by source read, nothing is compacted first); letters leave as aligned 8-byte stores, the bytes in
// front of the first and behind the last aligned unit of a read one by one.
__global__ __launch_bounds__(256) void k_un_unpack(const uint64_t *__restrict__ fwd, const uint64_t *__restrict__ amb,
						   const uint32_t *__restrict__ woff, const uint32_t *__restrict__ read_len,
						   const unsigned char *__restrict__ names, const uint32_t *__restrict__ name_at,
						   unsigned long long first_ordinal, const uint8_t *__restrict__ mask, const uint32_t *__restrict__ rank,
						   const uint64_t *__restrict__ let_off, const uint64_t *__restrict__ out_name_at, uint32_t n,
						   unsigned char *__restrict__ out_letters, unsigned char *__restrict__ out_names,
						   uint32_t *__restrict__ out_let_off32, uint32_t *__restrict__ out_name_at32)
{
	const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	const uint32_t r = (uint32_t)(t / kUnGroup), sub = (uint32_t)(t % kUnGroup);
	if (r > n)
		return;
	if (r == n) { // the closing offsets
		if (sub == 0) {
			out_let_off32[rank[n]] = (uint32_t)let_off[n];
			out_name_at32[rank[n]] = (uint32_t)out_name_at[n];
		}
		return;
	}
	if (!mask[r])
		return;
	const uint64_t D = let_off[r], NA = out_name_at[r];
	const uint32_t L = read_len[r], w0 = woff[r], nw = (L + 31) / 32;
	if (sub == 0) {
		out_let_off32[rank[r]] = (uint32_t)D;
		out_name_at32[rank[r]] = (uint32_t)NA;
	}
	// name
	if (name_at) {
		const uint32_t s = name_at[r], nb = name_at[r + 1] - s;
		for (uint32_t k = sub; k < nb; k += kUnGroup)
			out_names[NA + k] = names[s + k];
	} else if (sub == 0) {
		const uint32_t nb = (uint32_t)(out_name_at[r + 1] - NA);
		out_names[NA] = 'r';
		unsigned long long v = first_ordinal + r;
		for (uint32_t k = nb - 1; k >= 1; k--) {
			out_names[NA + k] = (unsigned char)('0' + v % 10);
			v /= 10;
		}
	}
	// 16 bits = 8 letters from letter i on
	auto bits_at = [&](const uint64_t *w, uint32_t i) -> uint32_t {
		const uint32_t k = i >> 5, sh = 2 * (i & 31);
		uint64_t v = w[w0 + k] >> sh;
		if (sh > 48 && k + 1 < nw)
			v |= w[w0 + k + 1] << (64 - sh);
		return (uint32_t)(v & 0xFFFFu);
	};
	auto letter = [](uint32_t base, uint32_t a) -> uint64_t { return (a & 1u) ? 'N' : (uint64_t)((0x54474341u >> (8 * (base & 3u))) & 0xFFu); };
	// letters in front of the first aligned unit, aligned units, letters behind the last
	const uint32_t head = (uint32_t)((8 - (D & 7)) & 7) < L ? (uint32_t)((8 - (D & 7)) & 7) : L;
	const uint32_t units = (L - head) / 8, tail0 = head + 8 * units;
	if (sub < head) {
		const uint32_t b = bits_at(fwd, sub), a = amb ? bits_at(amb, sub) : 0;
		out_letters[D + sub] = (unsigned char)letter(b, a);
	}
	for (uint32_t u = sub; u < units; u += kUnGroup) {
		const uint32_t i = head + 8 * u;
		const uint32_t b = bits_at(fwd, i), a = amb ? bits_at(amb, i) : 0;
		uint64_t v = 0;
#pragma unroll
		for (int k = 0; k < 8; k++)
			v |= letter(b >> (2 * k), a >> (2 * k)) << (8 * k);
		*reinterpret_cast<uint64_t *>(out_letters + D + i) = v;
	}
	if (tail0 + sub < L && sub < 8) {
		const uint32_t i = tail0 + sub;
		const uint32_t b = bits_at(fwd, i), a = amb ? bits_at(amb, i) : 0;
		out_letters[D + i] = (unsigned char)letter(b, a);
	}
}

template <typename T> static int exclusive_sum_on(const T *in, T *out, size_t n, hipStream_t st)
{
	size_t tmp_bytes = 0;
	PGX_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, in, out, T(0), n, rocprim::plus<T>(), st));
	DevBuf<uint8_t> tmp;
	PGX_TRY(tmp.alloc(tmp_bytes ? tmp_bytes : 1));
	PGX_HIP(rocprim::exclusive_scan(tmp.data(), tmp_bytes, in, out, T(0), n, rocprim::plus<T>(), st));
	PGX_HIP(hipStreamSynchronize(st)); // (tmp goes out of scope)
	return 0;
}

// ------------------------------------------------------------------------------------------ the script's options
struct UnParams {
	double t = 95, e = exp(-20.0), b = 200; // unclassified_selector.pl:28-30
};
static double num_of(const char *v) { return v ? perl_num(v, strlen(v)) : 0.0; } // (an undefined value numifies to 0)

// (name, percent, E, B) of a chomped table line: unclassified_selector.pl:85-95
static void un_cut(const std::string &line, std::string &name, double &percent, double &ev, double &bits)
{
	static const std::string tab = "\t";
	long start = p_index(line, tab, 0) + 1;
	start = p_index(line, tab, start) + 1;
	const long end = p_index(line, tab, start);
	percent = perl_num(p_substr(line, start, end - start));
	const long b_start = p_rindex(line, tab) + 1;
	bits = perl_num(p_substr(line, b_start, (long)line.size()));
	const long e_start = p_rindex(line, tab, b_start - 3) + 1;
	const long e_end = b_start - 1;
	ev = perl_num(p_substr(line, e_start, e_end - e_start));
	name = p_substr(line, 0, p_index(line, tab, 0));
}

} // namespace pgx

using namespace pgx;

extern "C" {

int pgx_unclas_file(int argc, const char *const *argv, char **log_text)
{
	Text log;
	return with_text(log, log_text, [&]() -> int {
		if (argc < 0 || (argc > 0 && !argv))
			return fail(PGX_E_ARG, "pgx_unclas_file: bad argument vector");
		return guard("pgx_unclas_file", [&]() -> int {
			if (argc - 1 < 5 || argc - 1 > 11) { // unclassified_selector.pl:21-25
				log.s += "Please enter the -m megablast, -s sequences, -t threshold, -e e-value upper threshold, -b bitscore lower "
					 "threshold, and -o output file.\n";
				return 0;
			}
			auto word = [&](int i) -> const char * { return i < argc ? argv[i] : nullptr; };
			UnParams p;
			const char *mega = nullptr, *sequ = nullptr, *outp = nullptr;
			for (int a = 0; a < 12; a++) { // :32-59: every position, values included
				const char *w = word(a);
				if (!w)
					continue;
				if (!strcmp(w, "-m"))
					mega = word(a + 1);
				else if (!strcmp(w, "-s"))
					sequ = word(a + 1);
				else if (!strcmp(w, "-t"))
					p.t = num_of(word(a + 1));
				else if (!strcmp(w, "-e"))
					p.e = exp(num_of(word(a + 1)));
				else if (!strcmp(w, "-b"))
					p.b = num_of(word(a + 1));
				else if (!strcmp(w, "-o"))
					outp = word(a + 1);
			}
			if (!(mega && sequ && outp)) { // :61-65
				log.s += "Must have at least -m megablast -s sequences -o output file.\n";
				return 0;
			}
			PGX_TRY(require_device());
			const char *hint = "\nMake sure you entered the extension when entering the file name.";
			bool ok;
			log.printf("Opening %s...", mega); // :67
			const std::string table = read_text_file(mega, &ok);
			if (!ok) {
				log.printf("Unable to open %s%s", mega, hint); // :70
				return 0;
			}
			log.s += "successful.\nRejecting...";
			// host: lines until the first empty one (:80), columns as the Perl would cut and numify them, interned names
			std::vector<double> pid, ev, bits;
			std::vector<uint32_t> row_name;
			std::unordered_map<std::string, uint32_t> name_id;
			std::string line, name;
			for (size_t s = 0; s < table.size();) {
				const size_t nl = table.find('\n', s);
				const size_t e = nl == std::string::npos ? table.size() : nl; // chomp: the newline only
				if (e == s && nl != std::string::npos)
					break;
				line.assign(table, s, e - s);
				s = nl == std::string::npos ? table.size() : e + 1;
				double a, b, c;
				un_cut(line, name, a, b, c);
				pid.push_back(a);
				ev.push_back(b);
				bits.push_back(c);
				row_name.push_back(name_id.emplace(name, (uint32_t)name_id.size()).first->second);
			}
			log.printf("successful.\nOpening %s...", sequ); // :115
			const std::string fasta = read_text_file(sequ, &ok);
			if (!ok) {
				log.printf("Unable to open %s%s", sequ, hint); // :118
				return 0;
			}
			log.printf("successful.\nCreating %s...", outp); // :122
			FILE *probe = fopen(outp, "w");
			if (!probe)
				return fail(PGX_E_IO, "%s: %s", outp, strerror(errno)); // :123 dies with $!
			fclose(probe);
			log.s += "successful.\nPrinting...";
			// FASTA lines: a line with '>' anywhere is a header (:128), its name the line without its first character and
			// without trailing white space (:130-131)
			struct Line {
				size_t start, len, name_len; // name at start + 1
			};
			std::vector<Line> lines;
			std::vector<uint32_t> hdr_name;
			for (size_t s = 0; s < fasta.size();) {
				const size_t nl = fasta.find('\n', s);
				const size_t e = nl == std::string::npos ? fasta.size() : nl + 1;
				Line ln{ s, e - s, 0 };
				uint32_t k = kNotHeader;
				if (memchr(fasta.data() + s, '>', e - s)) {
					size_t ne = e;
					while (ne > s + 1 && p_space(fasta[ne - 1]))
						ne--;
					ln.name_len = ne - (s + 1);
					auto it = name_id.find(fasta.substr(s + 1, ln.name_len));
					k = it == name_id.end() ? kNoName : it->second;
				}
				lines.push_back(ln);
				hdr_name.push_back(k);
				s = e;
			}
			if (lines.size() >= 0x7FFFFFFFull || name_id.size() >= kNotHeader)
				return fail(PGX_E_LIMIT, "pgx_unclas_file: 2^31 FASTA lines or more in one call");
			// device: row flags, OR per name, first header per name, fate per line
			const uint64_t n_rows = pid.size();
			const uint32_t n_lines = (uint32_t)lines.size();
			const size_t n_names = name_id.size();
			std::vector<uint32_t> fate(n_lines);
			if (n_lines) {
				DevBuf<double> d_pid, d_ev, d_bits;
				DevBuf<uint32_t> d_row_name, d_hdr, d_first, d_fate, d_run;
				DevBuf<uint8_t> d_pass, d_cls;
				PGX_TRY(d_pid.assign(pid));
				PGX_TRY(d_ev.assign(ev));
				PGX_TRY(d_bits.assign(bits));
				PGX_TRY(d_row_name.assign(row_name));
				PGX_TRY(d_hdr.assign(hdr_name));
				PGX_TRY(d_pass.alloc(n_rows ? n_rows : 1));
				PGX_TRY(d_cls.alloc(n_names ? n_names : 1, 0, 0, true));
				PGX_TRY(d_first.alloc(n_names ? n_names : 1));
				PGX_HIP(hipMemset(d_first.data(), 0xFF, (n_names ? n_names : 1) * sizeof(uint32_t)));
				PGX_TRY(d_fate.alloc(n_lines));
				PGX_TRY(d_run.alloc(n_lines));
				PGX_TRY(filter_lines_device(d_pid.data(), d_ev.data(), d_bits.data(), n_rows, p.t, p.e, p.b, d_pass.data(), 0));
				if (n_rows)
					hipLaunchKernelGGL(k_un_name_or, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, 0, d_pass.data(), d_row_name.data(),
							   n_rows, d_cls.data());
				const dim3 grid((n_lines + 255) / 256);
				hipLaunchKernelGGL(k_un_first_header, grid, dim3(256), 0, 0, d_hdr.data(), n_lines, d_first.data());
				hipLaunchKernelGGL(k_un_line_fate, grid, dim3(256), 0, 0, d_hdr.data(), d_cls.data(), d_first.data(), n_lines, d_fate.data());
				PGX_HIP(hipGetLastError());
				size_t tmp_bytes = 0;
				PGX_HIP(rocprim::inclusive_scan(nullptr, tmp_bytes, d_fate.data(), d_run.data(), (size_t)n_lines, rocprim::maximum<uint32_t>()));
				DevBuf<uint8_t> tmp;
				PGX_TRY(tmp.alloc(tmp_bytes ? tmp_bytes : 1));
				PGX_HIP(rocprim::inclusive_scan(tmp.data(), tmp_bytes, d_fate.data(), d_run.data(), (size_t)n_lines, rocprim::maximum<uint32_t>()));
				PGX_HIP(hipDeviceSynchronize());
				PGX_TRY(d_run.download(fate.data(), n_lines));
			}
			// the output from the kept line ranges (:136, :157, :164)
			std::string out;
			unsigned long long count = 0;
			for (uint32_t i = 0; i < n_lines; i++) {
				if (!(fate[i] & 1))
					continue;
				const Line &ln = lines[i];
				if (hdr_name[i] == kNotHeader) {
					out.append(fasta, ln.start, ln.len);
				} else {
					out += '>';
					out.append(fasta, ln.start + 1, ln.name_len);
					out += " \n";
					count++;
				}
			}
			PGX_TRY(write_text_file(outp, out));
			log.printf("successful.\nRejected %llu sequence(s).\nFinished!\n", count); // :167
			return 0;
		});
	});
}

int pgx_unclassified_batch(pgx_db *db, const pgx_reads *reads, const pgx_hits *hits, const pgx_unclas_opts *o, uint8_t *mask_out,
			   int64_t cap, int64_t *n_selected, pgx_reads **out)
{
	if (n_selected)
		*n_selected = 0;
	if (out)
		*out = nullptr;
	if (!db || !reads || !hits || !n_selected)
		return fail(PGX_E_ARG, "pgx_unclassified_batch: null argument");
	PGX_TRY(require_device());
	if (hits->n_reads != reads->n)
		return fail(PGX_E_ARG, "pgx_unclassified_batch: the table covers %lld reads, the batch holds %lld", (long long)hits->n_reads,
			    (long long)reads->n);
	if (mask_out && cap < reads->n)
		return fail(PGX_E_ARG, "pgx_unclassified_batch: mask buffer too small");
	if (reads->n >= 0x7FFFFFFFll)
		return fail(PGX_E_LIMIT, "pgx_unclassified_batch: 2^31 reads or more in one batch");
	return guard("pgx_unclassified_batch", [&]() -> int {
		UnParams p;
		if (o && o->t)
			p.t = num_of(o->t);
		if (o && o->e)
			p.e = exp(num_of(o->e));
		if (o && o->b)
			p.b = num_of(o->b);
		const uint32_t n = (uint32_t)reads->n;
		const bool have_names = !reads->synthetic;
		if (have_names && n && !reads->d_name_at.base)
			return fail(PGX_E_ARG, "pgx_unclassified_batch: the batch has no resident names");
		RowThresholds th;
		row_thresholds(p.t, p.e, p.b, db, reads, reads->n, hits->gapped, th);
		// duplicate read names: group ids (host), as pgx_megaclust_batch does
		std::vector<uint32_t> gid;
		if (have_names && !ReadNameIndex(*reads).unique) {
			std::unordered_map<std::string, uint32_t> ids;
			gid.resize(n);
			for (uint32_t r = 0; r < n; r++)
				gid[r] = ids.emplace(reads->name_of(r), (uint32_t)ids.size()).first->second;
		}
		std::lock_guard<std::mutex> lock(db->search_mu);
		hipStream_t st = nullptr;
		PGX_TRY(db_stream(db, &st));
		DevBuf<uint8_t> d_cls, d_mask, d_gcls;
		DevBuf<uint32_t> d_smin, d_gid, d_gfirst, d_add_rec, d_rank;
		DevBuf<uint64_t> d_add_let, d_add_name, d_let_off, d_name_off;
		PGX_TRY(d_cls.alloc(n ? n : 1, 0, 0, true));
		PGX_TRY(d_mask.alloc(n ? n : 1));
		PGX_TRY(d_smin.assign(th.s_min));
		PGX_TRY(d_add_rec.alloc((size_t)n + 1));
		PGX_TRY(d_rank.alloc((size_t)n + 1));
		PGX_TRY(d_add_let.alloc((size_t)n + 1));
		PGX_TRY(d_add_name.alloc((size_t)n + 1));
		PGX_TRY(d_let_off.alloc((size_t)n + 1));
		PGX_TRY(d_name_off.alloc((size_t)n + 1));
		const uint64_t n_slots = (uint64_t)hits->n_hits;
		if (n && n_slots) {
			const unsigned grid = (unsigned)std::min<uint64_t>((n_slots + 255) / 256, 256ull * 64);
			hipLaunchKernelGGL(k_un_rows, dim3(grid), dim3(256), 0, st, hits->d_hits.data(), n_slots, hits->d_read_off.data(),
					   hits->d_read_cnt.data(), reads->d_len.data(), n, th.h_min, d_smin.data(), th.max_len, d_cls.data());
			PGX_HIP(hipGetLastError());
		}
		if (!gid.empty()) {
			PGX_TRY(d_gid.assign(gid));
			PGX_TRY(d_gcls.alloc(n, 0, 0, true));
			PGX_TRY(d_gfirst.alloc(n));
			PGX_HIP(hipMemsetAsync(d_gfirst.data(), 0xFF, (size_t)n * sizeof(uint32_t), st));
			hipLaunchKernelGGL(k_un_group, dim3((n + 255) / 256), dim3(256), 0, st, d_cls.data(), d_gid.data(), n, d_gcls.data(), d_gfirst.data());
			PGX_HIP(hipGetLastError());
		}
		hipLaunchKernelGGL(k_un_mask, dim3((n + 1 + 255) / 256), dim3(256), 0, st, d_cls.data(), gid.empty() ? (const uint32_t *)nullptr : d_gid.data(),
				   d_gcls.data(), d_gfirst.data(), reads->d_len.data(), have_names ? reads->d_name_at.data() : (const uint32_t *)nullptr,
				   (unsigned long long)reads->first, n, d_mask.data(), d_add_rec.data(), d_add_let.data(), d_add_name.data());
		PGX_HIP(hipGetLastError());
		PGX_TRY(exclusive_sum_on(d_add_rec.data(), d_rank.data(), (size_t)n + 1, st));
		uint32_t n_sel = 0;
		PGX_TRY(d_rank.download(&n_sel, 1, n));
		*n_selected = n_sel;
		if (mask_out)
			PGX_TRY(d_mask.download(mask_out, n));
		if (!out)
			return 0;
		// the subset batch: letters and names of the selected reads as the records of a DeviceFasta
		PGX_TRY(exclusive_sum_on(d_add_let.data(), d_let_off.data(), (size_t)n + 1, st));
		PGX_TRY(exclusive_sum_on(d_add_name.data(), d_name_off.data(), (size_t)n + 1, st));
		uint64_t letters = 0, name_bytes = 0;
		PGX_TRY(d_let_off.download(&letters, 1, n));
		PGX_TRY(d_name_off.download(&name_bytes, 1, n));
		if (letters >= (1ull << 32) || name_bytes >= (1ull << 32))
			return fail(PGX_E_LIMIT, "pgx_unclassified_batch: 2^32 letters or name bytes and more in the selected reads: use smaller batches");
		DeviceFasta df;
		DevBuf<uint32_t> d_let_off32;
		PGX_TRY(df.d_letters.alloc(letters ? letters : 1, 0, 16));
		PGX_TRY(df.d_names.alloc(name_bytes ? name_bytes : 1, 0, 16));
		PGX_TRY(df.d_name_at.alloc((size_t)n_sel + 1));
		PGX_TRY(d_let_off32.alloc((size_t)n_sel + 1));
		{
			const uint64_t lanes = ((uint64_t)n + 1) * kUnGroup;
			hipLaunchKernelGGL(k_un_unpack, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, reads->d_fwd.data(),
					   reads->has_amb ? reads->d_fwd_amb.data() : (const uint64_t *)nullptr, reads->d_woff.data(), reads->d_len.data(),
					   have_names ? reads->d_names.data() : (const unsigned char *)nullptr,
					   have_names ? reads->d_name_at.data() : (const uint32_t *)nullptr, (unsigned long long)reads->first, d_mask.data(),
					   d_rank.data(), d_let_off.data(), d_name_off.data(), n, df.d_letters.data(), df.d_names.data(), d_let_off32.data(),
					   df.d_name_at.data());
			PGX_HIP(hipGetLastError());
			PGX_HIP(hipStreamSynchronize(st));
		}
		trace_point("unclassified: unpacked");
		df.let_off.resize((size_t)n_sel + 1);
		df.name_at.resize((size_t)n_sel + 1);
		PGX_TRY(d_let_off32.download(df.let_off.data(), (size_t)n_sel + 1));
		PGX_TRY(df.d_name_at.download(df.name_at.data(), (size_t)n_sel + 1));
		df.names.resize(name_bytes);
		if (name_bytes)
			PGX_TRY(df.d_names.download((unsigned char *)&df.names[0], name_bytes));
		// (the scans and flags are let go before the import's second half allocates the batch)
		d_cls.release();
		d_add_rec.release();
		d_rank.release();
		d_add_let.release();
		d_add_name.release();
		d_let_off.release();
		d_name_off.release();
		d_let_off32.release();
		std::unique_ptr<pgx_reads> rd;
		PGX_TRY(reads_from_device_fasta(df, 0, -1, false, nullptr, rd));
		*out = rd.release();
		return 0;
	});
}
}
