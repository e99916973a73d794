// Barcode/barcode.pl (the step before Trim): a 454-style FASTA split into one FASTA per sample barcode, the
// barcode cut off, reads left too short thrown out.  The rule, with the script's accidents, is tests/barcode_rule.py.
//
//   pgx_barcode_file     the reference command line: stdout text, and in -d one bar<name>.fas per barcode, nobar.fas,
//                        barcode_count.txt, info.txt
//   pgx_barcode_reads    the same run with the output kept in HBM: each barcode's FASTA is a slice of one buffer, and
//                        pgx_barcodes_take_reads sends a slice through the device FASTA splitter into a read batch
//
// Device: the text's line index (k_nl_count / k_nl_write, trim.hip), which lines hold '>' (k_bc_gt) and which are the empty
// line (k_bc_lines), the header lines in order (a scan), one wavefront per record for the search (k_bc_match), a stable
// sort of the records by destination and a scan of their sizes, one wavefront per record for the copy (k_bc_write).
// Host: the barcode file, the file's last record (barcode_host.hpp), the two small text files, the stdout text.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <cerrno>
#include <cstring>

#include "barcode_host.hpp"
#include "engine.hpp"

namespace pgx {

// one barcode as the search reads it from LDS: its first 8 letters as one word (zero-filled), its length
struct BcEntry {
	uint64_t w8;
	uint32_t len, pad;
};
constexpr int kBcStride = (int)kBcMaxLetters; // letters of barcode a at letters[a * kBcStride], for the ones longer than 8
constexpr uint32_t kBcThreads = 256, kBcWaves = kBcThreads / 64;

// 8 bytes at any offset from two aligned 8-byte loads (the text has 32 readable bytes behind its end)
__device__ __forceinline__ uint64_t bc_load8(const uint8_t *__restrict__ text, uint64_t off)
{
	const uint64_t *p = reinterpret_cast<const uint64_t *>(text + (off & ~7ull));
	const uint32_t sh = (uint32_t)(off & 7) * 8;
	const uint64_t a = p[0], b = p[1];
	return sh ? (a >> sh) | (b << (64 - sh)) : a;
}
__device__ __forceinline__ uint64_t bc_mask(uint32_t len) { return len >= 8 ? ~0ull : (1ull << (8 * len)) - 1; }

// letters 8.. of a barcode against the text (the masked word has matched)
__device__ __forceinline__ bool bc_tail_eq(const uint8_t *__restrict__ t, const uint8_t *__restrict__ w, uint32_t len)
{
	for (uint32_t k = 8; k < len; k++)
		if (t[k] != w[k])
			return false;
	return true;
}

// hdr[line] = 1 for every line that holds a '>' anywhere (barcode.pl:96): 16 bytes per lane, the rare '>' looks its line
// up in the index
__global__ __launch_bounds__(256) void k_bc_gt(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ start, uint64_t n_lines,
					       uint32_t *__restrict__ hdr)
{
	for (uint64_t off = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16; off < n; off += (uint64_t)gridDim.x * 256 * 16) {
		const uint4 v = *reinterpret_cast<const uint4 *>(text + off); // (padding behind the text)
		const uint32_t w[4] = { v.x, v.y, v.z, v.w };
		for (int q = 0; q < 4; q++) {
			const uint32_t x = w[q] ^ 0x3E3E3E3Eu;
			if (!((x - 0x01010101u) & ~x & 0x80808080u))
				continue;
			for (int k = 0; k < 4; k++) {
				const uint64_t at = off + 4 * q + k;
				if (at >= n || ((w[q] >> (8 * k)) & 0xFF) != '>')
					continue;
				uint64_t lo = 0, hi = n_lines; // last line with start <= at
				while (hi - lo > 1) {
					const uint64_t mid = (lo + hi) / 2;
					if (start[mid] <= at)
						lo = mid;
					else
						hi = mid;
				}
				hdr[lo] = 1;
			}
		}
	}
}

// empt[line] = 1 for a line that is exactly "\n" and no header (:109: it is not stored).  n_lines + 1 entries, the last 0.
__global__ void k_bc_lines(const uint8_t *__restrict__ text, const uint64_t *__restrict__ start, uint64_t n_lines, uint32_t *__restrict__ empt)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i > n_lines)
		return;
	empt[i] = i < n_lines && start[i + 1] - start[i] == 1 && text[start[i]] == '\n';
}

// hdr_line[rank[i]] = i for the header lines; a stored line in front of the first header raises `stray` (refused)
__global__ void k_bc_headers(const uint32_t *__restrict__ hdr, const uint32_t *__restrict__ rank, const uint32_t *__restrict__ empt, uint64_t n_lines,
			     uint32_t *__restrict__ hdr_line, uint32_t *__restrict__ stray)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i > n_lines)
		return;
	if (i == n_lines) {
		hdr_line[rank[i]] = (uint32_t)n_lines; // closes the last record
		return;
	}
	if (hdr[i])
		hdr_line[rank[i]] = (uint32_t)i;
	else if (rank[i] == 0 && !empt[i])
		*stray = 1;
}

struct BcRecs { // per record
	uint32_t *dest;    // 0 nobar, 1 + a barcode a, n_bars + 1 thrown out
	uint64_t *begin;   // the bytes copied behind the (rewritten) header: [begin, end) without its empty lines
	uint64_t *end;
	uint64_t *size;    // bytes written
	uint32_t *pushed;  // lines the script pushes onto the barcode's list
};

// barcode.pl:164-211 and :258-268 for every record but the file's last: one wavefront per record.  Per stored line, in
// order: every barcode as a prefix (lanes over barcodes, the lowest set bit of the ballot wins: place = 1 whatever the
// line), else every barcode in file order as a substring (lanes over line positions, a wave-uniform loop over barcodes that
// ends at the first one with a hit anywhere in the line).  The first line with a match ends the search.
__global__ __launch_bounds__(kBcThreads) void k_bc_match(const uint8_t *__restrict__ text, const uint64_t *__restrict__ start,
							  const uint32_t *__restrict__ hdr_line, const uint32_t *__restrict__ empt_ex, uint32_t n_rec,
							  const BcEntry *__restrict__ bars, const uint8_t *__restrict__ letters,
							  const uint32_t *__restrict__ name_len, uint32_t n_bars, BcRecs out)
{
	extern __shared__ BcEntry s_bar[];
	for (uint32_t i = threadIdx.x; i < n_bars; i += kBcThreads)
		s_bar[i] = bars[i];
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (uint64_t r = (uint64_t)blockIdx.x * kBcWaves + wave; r < n_rec; r += (uint64_t)gridDim.x * kBcWaves) {
		const uint32_t l0 = hdr_line[r], l1 = hdr_line[r + 1];
		int found = -1;
		long long idx = 0;             // index(line[place], barcode)
		uint32_t place_line = 0, first_line = 0, b = 0;
		for (uint32_t i = l0 + 1; i < l1 && found < 0; i++) {
			if (empt_ex[i + 1] != empt_ex[i])
				continue;
			const uint64_t lo = start[i], ln = start[i + 1] - lo;
			if (++b == 1)
				first_line = i;
			// prefix
			const uint64_t w0 = bc_load8(text, lo);
			for (uint32_t base = 0; base < n_bars && found < 0; base += 64) {
				const uint32_t a = base + lane;
				bool hit = false;
				if (a < n_bars) {
					const BcEntry e = s_bar[a];
					hit = e.len <= ln && ((w0 ^ e.w8) & bc_mask(e.len)) == 0 &&
					      (e.len <= 8 || bc_tail_eq(text + lo, letters + (size_t)a * kBcStride, e.len));
				}
				const uint64_t m = __ballot(hit);
				if (m)
					found = (int)(base + (uint32_t)__ffsll((long long)m) - 1);
			}
			if (found >= 0) {
				place_line = first_line;
				idx = b == 1 ? 0 : -1; // a prefix on a later line: line 1 holds no barcode at all
				break;
			}
			// substring
			uint32_t best = n_bars;
			for (uint64_t p0 = 0; p0 < ln; p0 += 64) {
				const uint64_t p = p0 + lane;
				const uint64_t w = p < ln ? bc_load8(text, lo + p) : 0;
				for (uint32_t a = 0; a < best; a++) {
					const BcEntry e = s_bar[a];
					const bool hit = p + e.len <= ln && ((w ^ e.w8) & bc_mask(e.len)) == 0 &&
							 (e.len <= 8 || bc_tail_eq(text + lo + p, letters + (size_t)a * kBcStride, e.len));
					if (__ballot(hit)) {
						best = a;
						break;
					}
				}
			}
			if (best < n_bars) {
				found = (int)best;
				place_line = i;
				const BcEntry e = s_bar[best];
				for (uint64_t p0 = 0; p0 < ln; p0 += 64) { // its leftmost occurrence
					const uint64_t p = p0 + lane;
					const bool hit = p + e.len <= ln && ((bc_load8(text, p < ln ? lo + p : lo) ^ e.w8) & bc_mask(e.len)) == 0 &&
							 (e.len <= 8 || bc_tail_eq(text + lo + p, letters + (size_t)best * kBcStride, e.len));
					const uint64_t m = __ballot(hit);
					if (m) {
						idx = (long long)(p0 + (uint64_t)__ffsll((long long)m) - 1);
						break;
					}
				}
			}
		}
		if (lane != 0)
			continue;
		const uint64_t rec_begin = start[l0], rec_end = start[l1];
		const uint32_t e_end = empt_ex[l1];
		uint32_t dest = 0, pushed = 0;
		uint64_t begin = rec_begin, size = (rec_end - rec_begin) - (e_end - empt_ex[l0]) + 1; // no barcode: the record and "\n"
		if (found >= 0) {
			const uint32_t len = s_bar[found].len;
			const uint64_t lo = start[place_line], ln = start[place_line + 1] - lo;
			const uint64_t after = (rec_end - start[place_line + 1]) - (e_end - empt_ex[place_line + 1]); // lengths of the lines behind `place`
			const long long bases = 60 - (idx + (long long)len) + (long long)after; // (60 is the script's constant, not the line's length)
			if (bases < 100) {
				dest = n_bars + 1;
				begin = rec_end;
				size = 0;
			} else {
				const uint64_t past = (uint64_t)(idx + (long long)len), cut = past < ln ? past : ln;
				dest = 1 + (uint32_t)found;
				begin = lo + cut;
				size = (start[l0 + 1] - rec_begin) + name_len[found] + 1 + (ln - cut) + after + 1;
				pushed = 2 + (l1 - place_line) - (e_end - empt_ex[place_line]);
			}
		}
		out.dest[r] = dest;
		out.begin[r] = begin;
		out.end[r] = rec_end;
		out.size[r] = size;
		out.pushed[r] = pushed;
	}
}

// bytes, records and pushed lines per destination
__global__ void k_bc_totals(BcRecs rec, uint32_t n_rec, unsigned long long *__restrict__ d_bytes, unsigned long long *__restrict__ d_recs,
			    unsigned long long *__restrict__ d_pushed)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_rec)
		return;
	const uint32_t d = rec.dest[r];
	atomicAdd(&d_bytes[d], (unsigned long long)rec.size[r]);
	atomicAdd(&d_recs[d], 1ull);
	atomicAdd(&d_pushed[d], (unsigned long long)rec.pushed[r]);
}

__global__ void k_bc_iota(uint32_t *__restrict__ v, uint32_t n)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n)
		v[i] = i;
}
__global__ void k_bc_gather(const uint64_t *__restrict__ size, const uint32_t *__restrict__ order, uint32_t n, uint64_t *__restrict__ sorted_size)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j < n)
		sorted_size[j] = size[order[j]];
}
__global__ void k_bc_scatter(const uint64_t *__restrict__ sorted_off, const uint32_t *__restrict__ order, uint32_t n, uint64_t *__restrict__ out_off)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j < n)
		out_off[order[j]] = sorted_off[j];
}

// barcode.pl:212-255: one wavefront per record.  A kept read: ">" name "_" header[1:], the bytes [begin, end) -- the
// barcode line from behind the barcode, the later lines whole -- and "\n"; a read with no barcode: its lines and "\n".
// A byte '\n' that follows a '\n' is an empty line, which the script never stored: left out by a ballot compaction.
__global__ __launch_bounds__(kBcThreads) void k_bc_write(const uint8_t *__restrict__ text, const uint64_t *__restrict__ start,
							  const uint32_t *__restrict__ hdr_line, uint32_t n_rec, uint32_t n_bars, BcRecs rec,
							  const uint64_t *__restrict__ out_off, const uint8_t *__restrict__ names,
							  const uint32_t *__restrict__ name_at, uint8_t *__restrict__ out)
{
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (uint64_t r = (uint64_t)blockIdx.x * kBcWaves + wave; r < n_rec; r += (uint64_t)gridDim.x * kBcWaves) {
		const uint32_t dest = rec.dest[r];
		if (dest > n_bars)
			continue;
		uint64_t o = out_off[r];
		if (dest > 0) {
			const uint32_t l0 = hdr_line[r];
			const uint64_t h = start[l0], hl = start[l0 + 1] - h;
			const uint32_t ns = name_at[dest - 1], nl = name_at[dest] - ns;
			if (lane == 0)
				out[o] = '>';
			for (uint32_t k = lane; k < nl; k += 64)
				out[o + 1 + k] = names[ns + k];
			if (lane == 0)
				out[o + 1 + nl] = '_';
			for (uint64_t k = 1 + lane; k < hl; k += 64)
				out[o + 1 + nl + k] = text[h + k];
			o += hl + nl + 1;
		}
		const uint64_t begin = rec.begin[r], end = rec.end[r];
		for (uint64_t p0 = begin; p0 < end; p0 += 64) {
			const uint64_t p = p0 + lane;
			uint8_t c = 0;
			bool keep = false;
			if (p < end) {
				c = text[p];
				keep = !(c == '\n' && p > 0 && text[p - 1] == '\n');
			}
			const uint64_t m = __ballot(keep);
			if (keep)
				out[o + __popcll(m & ((1ull << lane) - 1))] = c;
			o += __popcll(m);
		}
		if (lane == 0)
			out[o] = '\n';
	}
}

template <typename In, typename Out> static int bc_exclusive_sum(const In *in, Out *out, size_t n)
{
	size_t bytes = 0;
	PGX_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, (Out)0, n, rocprim::plus<Out>()));
	DevBuf<uint8_t> tmp;
	PGX_TRY(tmp.alloc(bytes ? bytes : 1));
	PGX_HIP(rocprim::exclusive_scan(tmp.data(), bytes, in, out, (Out)0, n, rocprim::plus<Out>()));
	PGX_HIP(hipDeviceSynchronize()); // (tmp goes out of scope)
	return 0;
}

} // namespace pgx

// What a run leaves: the barcodes, the counts, and every output FASTA as a slice of one buffer in HBM
struct pgx_barcodes {
	std::vector<pgx::BcBar> bars;
	std::vector<uint64_t> slice;  // n_bars + 2 offsets into `out`: nobar, then one per barcode
	std::vector<uint64_t> recs;   // n_bars + 2 record counts: nobar, barcodes, thrown out
	std::vector<uint64_t> pushed; // lines pushed per destination (info.txt starts from barcode 1's)
	uint64_t n_seq = 0;           // header lines
	pgx::DevBuf<uint8_t> out;
};

namespace pgx {

static unsigned bc_grid(uint64_t n_rec) { return (unsigned)std::min<uint64_t>((n_rec + kBcWaves - 1) / kBcWaves, 256u * 16u); }

// the whole run on the text of the sequence file
static int barcode_run(const std::string &text, const std::vector<BcBar> &bars, pgx_barcodes &res)
{
	const uint32_t nb = (uint32_t)bars.size();
	const uint64_t n = text.size();
	res.slice.assign((size_t)nb + 2, 0);
	res.recs.assign((size_t)nb + 2, 0);
	res.pushed.assign((size_t)nb + 2, 0);
	res.n_seq = 0;
	// the last record, and the line count of the one before it: host
	std::vector<BcLine> last;
	uint64_t stale = 0;
	const bool any_header = bc_tail_records(text.data(), n, last, stale);
	if (!any_header) {
		for (uint64_t k = 0; k < n; k++) // (no '>' in the text: one pass over what must be empty lines)
			if (text[k] != '\n')
				return fail(PGX_E_ARG, "pgx_barcode: text before the first header line");
		res.recs[nb + 1] = 1; // barcode.pl:116 on the empty list: "thrown out"
		return res.out.alloc(1, 0, 32);
	}
	const BcFate lf = bc_last_record(text.data(), last, bars, stale);
	if (lf.status < 0)
		return fail(lf.status, "pgx_barcode: the reference script never ends on the last record of this file (a barcode heads one of its lines "
				       "behind the line count of the record before it)");
	// text and line index
	DevBuf<uint8_t> d_text;
	DevBuf<uint64_t> d_start;
	uint64_t n_lines = 0;
	PGX_TRY(d_text.alloc(n, 0, 32));
	PGX_TRY(d_text.upload((const uint8_t *)text.data(), n));
	PGX_TRY(device_line_index(d_text.data(), n, text[n - 1] != '\n', d_start, &n_lines));
	if (n_lines >= 0x7FFFFFFFull)
		return fail(PGX_E_LIMIT, "pgx_barcode: 2^31 lines or more in one call");
	// header lines, empty lines, records
	DevBuf<uint32_t> d_hdr, d_rank, d_empt, d_empt_ex, d_hdr_line, d_stray;
	PGX_TRY(d_hdr.alloc(n_lines + 1, 0, 0, true));
	PGX_TRY(d_rank.alloc(n_lines + 1));
	PGX_TRY(d_empt.alloc(n_lines + 1));
	PGX_TRY(d_empt_ex.alloc(n_lines + 1));
	PGX_TRY(d_stray.alloc(1, 0, 0, true));
	const unsigned g_lines = (unsigned)((n_lines + 1 + 255) / 256);
	hipLaunchKernelGGL(k_bc_gt, dim3((unsigned)std::min<uint64_t>((n + 4095) / 4096, 256u * 32u)), dim3(256), 0, 0, d_text.data(), n, d_start.data(),
			   n_lines, d_hdr.data());
	hipLaunchKernelGGL(k_bc_lines, dim3(g_lines), dim3(256), 0, 0, d_text.data(), d_start.data(), n_lines, d_empt.data());
	PGX_HIP(hipGetLastError());
	PGX_TRY((bc_exclusive_sum<uint32_t, uint32_t>(d_hdr.data(), d_rank.data(), (size_t)n_lines + 1)));
	PGX_TRY((bc_exclusive_sum<uint32_t, uint32_t>(d_empt.data(), d_empt_ex.data(), (size_t)n_lines + 1)));
	uint32_t n_rec = 0;
	PGX_TRY(d_rank.download(&n_rec, 1, n_lines));
	PGX_TRY(d_hdr_line.alloc((size_t)n_rec + 1));
	hipLaunchKernelGGL(k_bc_headers, dim3(g_lines), dim3(256), 0, 0, d_hdr.data(), d_rank.data(), d_empt.data(), n_lines, d_hdr_line.data(),
			   d_stray.data());
	PGX_HIP(hipGetLastError());
	uint32_t stray = 0;
	PGX_TRY(d_stray.download(&stray, 1));
	if (stray)
		return fail(PGX_E_ARG, "pgx_barcode: text before the first header line");
	if (n_rec == 0)
		return fail(PGX_E_FORMAT, "pgx_barcode: the line index found no header line");
	d_hdr.release();
	d_rank.release();
	d_empt.release();
	res.n_seq = n_rec;
	// barcodes: the LDS table, the letters, the names
	std::vector<BcEntry> h_bar(nb ? nb : 1);
	std::vector<uint8_t> h_letters((size_t)(nb ? nb : 1) * kBcStride, 0), h_names;
	std::vector<uint32_t> h_name_at(1, 0), h_name_len(nb ? nb : 1, 0);
	for (uint32_t a = 0; a < nb; a++) {
		const std::string &w = bars[a].letters;
		memcpy(&h_letters[(size_t)a * kBcStride], w.data(), w.size());
		uint64_t w8 = 0;
		memcpy(&w8, w.data(), std::min<size_t>(8, w.size()));
		h_bar[a] = BcEntry{ w8, (uint32_t)w.size(), 0 };
		h_names.insert(h_names.end(), bars[a].name.begin(), bars[a].name.end());
		h_name_at.push_back((uint32_t)h_names.size());
		h_name_len[a] = (uint32_t)bars[a].name.size();
	}
	DevBuf<BcEntry> d_bar;
	DevBuf<uint8_t> d_letters, d_names;
	DevBuf<uint32_t> d_name_at, d_name_len;
	PGX_TRY(d_bar.assign(h_bar));
	PGX_TRY(d_letters.assign(h_letters));
	PGX_TRY(d_names.assign(h_names));
	PGX_TRY(d_name_at.assign(h_name_at));
	PGX_TRY(d_name_len.assign(h_name_len));
	// per record: fate and sizes; the last record's are the host's
	DevBuf<uint32_t> d_dest, d_pushed;
	DevBuf<uint64_t> d_begin, d_end, d_size;
	PGX_TRY(d_dest.alloc(n_rec));
	PGX_TRY(d_pushed.alloc(n_rec));
	PGX_TRY(d_begin.alloc(n_rec));
	PGX_TRY(d_end.alloc(n_rec));
	PGX_TRY(d_size.alloc(n_rec));
	const BcRecs rec{ d_dest.data(), d_begin.data(), d_end.data(), d_size.data(), d_pushed.data() };
	if (n_rec > 1) {
		hipLaunchKernelGGL(k_bc_match, dim3(bc_grid(n_rec - 1)), dim3(kBcThreads), (size_t)nb * sizeof(BcEntry), 0, d_text.data(), d_start.data(),
				   d_hdr_line.data(), d_empt_ex.data(), n_rec - 1, d_bar.data(), d_letters.data(), d_name_len.data(), nb, rec);
		PGX_HIP(hipGetLastError());
	}
	{
		const uint32_t dest = lf.bar < 0 ? 0u : lf.kept ? 1u + (uint32_t)lf.bar : nb + 1;
		const uint64_t size = dest <= nb ? lf.size : 0;
		const uint32_t r = n_rec - 1;
		PGX_HIP(hipMemcpy(d_dest.data() + r, &dest, sizeof dest, hipMemcpyHostToDevice));
		PGX_HIP(hipMemcpy(d_begin.data() + r, &lf.body_begin, sizeof(uint64_t), hipMemcpyHostToDevice));
		PGX_HIP(hipMemcpy(d_end.data() + r, &lf.body_end, sizeof(uint64_t), hipMemcpyHostToDevice));
		PGX_HIP(hipMemcpy(d_size.data() + r, &size, sizeof size, hipMemcpyHostToDevice));
		PGX_HIP(hipMemcpy(d_pushed.data() + r, &lf.pushed, sizeof(uint32_t), hipMemcpyHostToDevice));
	}
	trace_point("barcode: match");
	// placement: records in destination order (stable: input order within a file), offsets from a scan of their sizes
	const unsigned g_rec = (n_rec + 255) / 256;
	DevBuf<unsigned long long> d_tot;
	PGX_TRY(d_tot.alloc(3 * ((size_t)nb + 2), 0, 0, true));
	hipLaunchKernelGGL(k_bc_totals, dim3(g_rec), dim3(256), 0, 0, rec, n_rec, d_tot.data(), d_tot.data() + (nb + 2), d_tot.data() + 2 * (nb + 2));
	DevBuf<uint32_t> d_iota, d_order, d_key_out;
	DevBuf<uint64_t> d_sorted_size, d_sorted_off, d_out_off;
	PGX_TRY(d_iota.alloc(n_rec));
	PGX_TRY(d_order.alloc(n_rec));
	PGX_TRY(d_key_out.alloc(n_rec));
	PGX_TRY(d_sorted_size.alloc(n_rec));
	PGX_TRY(d_sorted_off.alloc(n_rec));
	PGX_TRY(d_out_off.alloc(n_rec));
	hipLaunchKernelGGL(k_bc_iota, dim3(g_rec), dim3(256), 0, 0, d_iota.data(), n_rec);
	PGX_HIP(hipGetLastError());
	{
		unsigned key_bits = 1;
		while ((1u << key_bits) < nb + 2)
			key_bits++;
		size_t bytes = 0;
		PGX_HIP(rocprim::radix_sort_pairs(nullptr, bytes, d_dest.data(), d_key_out.data(), d_iota.data(), d_order.data(), (size_t)n_rec, 0, key_bits));
		DevBuf<uint8_t> tmp;
		PGX_TRY(tmp.alloc(bytes ? bytes : 1));
		PGX_HIP(rocprim::radix_sort_pairs(tmp.data(), bytes, d_dest.data(), d_key_out.data(), d_iota.data(), d_order.data(), (size_t)n_rec, 0, key_bits));
		PGX_HIP(hipDeviceSynchronize());
	}
	hipLaunchKernelGGL(k_bc_gather, dim3(g_rec), dim3(256), 0, 0, d_size.data(), d_order.data(), n_rec, d_sorted_size.data());
	PGX_HIP(hipGetLastError());
	PGX_TRY((bc_exclusive_sum<uint64_t, uint64_t>(d_sorted_size.data(), d_sorted_off.data(), (size_t)n_rec)));
	hipLaunchKernelGGL(k_bc_scatter, dim3(g_rec), dim3(256), 0, 0, d_sorted_off.data(), d_order.data(), n_rec, d_out_off.data());
	PGX_HIP(hipGetLastError());
	std::vector<unsigned long long> tot(3 * ((size_t)nb + 2));
	PGX_TRY(d_tot.download(tot.data(), tot.size()));
	uint64_t total = 0;
	for (uint32_t d = 0; d < nb + 2; d++) {
		if (d <= nb) {
			res.slice[d] = total;
			total += tot[d];
		}
		res.recs[d] = tot[(nb + 2) + d];
		res.pushed[d] = tot[2 * (nb + 2) + d];
	}
	res.slice[nb + 1] = total;
	PGX_TRY(res.out.alloc(total, 0, 32));
	hipLaunchKernelGGL(k_bc_write, dim3(bc_grid(n_rec)), dim3(kBcThreads), 0, 0, d_text.data(), d_start.data(), d_hdr_line.data(), n_rec, nb, rec,
			   d_out_off.data(), d_names.data(), d_name_at.data(), res.out.data());
	PGX_HIP(hipGetLastError());
	PGX_HIP(hipDeviceSynchronize());
	trace_point("barcode: write");
	return 0;
}

// both inputs read and the barcode file parsed; the messages of barcode.pl:51-66 go to `log` when there is one
static int barcode_inputs(const char *seq, const char *bar, Text *log, std::string &text, std::vector<BcBar> &bars, bool &opened)
{
	const char *hint = "\nMake sure you entered the extension when entering the file name.";
	opened = false;
	bool ok;
	if (log)
		log->printf("Opening %s...", seq);
	text = read_text_file(seq, &ok);
	if (!ok) {
		if (log)
			log->printf("Unable to open %s%s", seq, hint);
		return log ? 0 : fail(PGX_E_IO, "cannot open %s", seq);
	}
	if (log)
		log->printf("Successful.\nOpening %s...", bar);
	const std::string btext = read_text_file(bar, &ok);
	if (!ok) {
		if (log)
			log->printf("Unable to open %s%s", bar, hint);
		return log ? 0 : fail(PGX_E_IO, "cannot open %s", bar);
	}
	if (log)
		log->s += "Successful.\nCreating Files...\n";
	opened = true;
	std::string why;
	const int rc = bc_parse_barcodes(btext, bars, why);
	if (rc < 0)
		return fail(rc, "pgx_barcode: %s", why.c_str());
	return 0;
}

} // namespace pgx

using namespace pgx;

extern "C" {

int pgx_barcode_file(int argc, const char *const *argv, char **log_text)
{
	Text log;
	return with_text(log, log_text, [&]() -> int {
		if (argc < 0 || (argc > 0 && !argv))
			return fail(PGX_E_ARG, "pgx_barcode_file: bad argument vector");
		return guard("pgx_barcode_file", [&]() -> int {
			if (argc - 1 < 3) { // barcode.pl:18
				log.s += "Please enter the -s sequences and -b barcodes.\n";
				return 0;
			}
			if (argc - 1 > 5) { // :23
				log.s += "Too many inputs\n";
				return 0;
			}
			auto word = [&](int i) -> const char * { return i < argc ? argv[i] : nullptr; };
			const char *seq = nullptr, *bar = nullptr, *dir = nullptr;
			for (int a = 0; a < argc; a++) { // :29-43: every position, values included
				if (!strcmp(argv[a], "-s"))
					seq = word(a + 1);
				else if (!strcmp(argv[a], "-b"))
					bar = word(a + 1);
				else if (!strcmp(argv[a], "-d"))
					dir = word(a + 1);
			}
			if (!seq || !bar) { // :45
				log.s += "Must enter at least -s sequences and -b barcodes.\n";
				return 0;
			}
			if (!dir)
				return fail(PGX_E_ARG, "pgx_barcode_file: no -d directory (the script would write /info.txt)");
			PGX_TRY(require_device());
			std::string text;
			std::vector<BcBar> bars;
			bool opened;
			Text head;
			const int irc = barcode_inputs(seq, bar, &head, text, bars, opened);
			if (irc < 0)
				return irc; // refused: nothing printed, nothing written
			log.s += head.s;
			if (!opened)
				return 0;
			pgx_barcodes res;
			res.bars = bars;
			{
				const int rc = barcode_run(text, bars, res);
				if (rc < 0) {
					log.s.clear();
					return rc;
				}
			}
			const uint32_t nb = (uint32_t)bars.size();
			const uint64_t total = res.slice[nb + 1];
			std::string out(total, '\0');
			if (total)
				PGX_TRY(res.out.download((uint8_t *)&out[0], total));
			const std::string d = std::string(dir) + "/";
			auto put = [&](const std::string &name, const std::string &s) -> int {
				const std::string path = d + name;
				FILE *f = fopen(path.c_str(), "wb");
				if (!f)
					return fail(PGX_E_IO, "%s: %s", path.c_str(), strerror(errno)); // the script dies with $!
				const bool ok = fwrite(s.data(), 1, s.size(), f) == s.size();
				if (fclose(f) != 0 || !ok)
					return fail(PGX_E_IO, "%s: write failed", path.c_str());
				return 0;
			};
			PGX_TRY(put("nobar.fas", out.substr(res.slice[0], res.slice[1] - res.slice[0])));
			Text count;
			unsigned long long norm = 0, mn = nb ? res.pushed[1] : 0; // :119: a count of pushed lines
			for (uint32_t a = 0; a < nb; a++) {
				const unsigned long long c = res.recs[1 + a];
				norm += c;
				count.printf("%02u\t%s\t%llu\n", a + 1, bars[a].letters.c_str(), c); // :125-132
				PGX_TRY(put("bar" + bars[a].name + ".fas", out.substr(res.slice[1 + a], res.slice[2 + a] - res.slice[1 + a])));
				if (c > 100 && c < mn) // :145-151
					mn = c;
			}
			PGX_TRY(put("barcode_count.txt", count.s));
			PGX_TRY(put("info.txt", std::to_string(mn)));
			log.printf("Found %llu sequences.\nFound %s barcodes at the beginning.\nFound no barcodes in %llu sequences.\n"
				   "Threw out %llu barcodes based on length.\nWriting Files...Successful.\nFinished!\n",
				   (unsigned long long)res.n_seq, norm ? std::to_string(norm).c_str() : "", (unsigned long long)res.recs[0],
				   (unsigned long long)res.recs[nb + 1]); // :118, :156 ($countNorm is undefined until a barcode is found)
			return 0;
		});
	});
}

int pgx_barcode_reads(const char *reads_path, const char *barcodes_path, pgx_barcodes **out)
{
	if (out)
		*out = nullptr;
	PGX_TRY(require_device());
	if (!reads_path || !barcodes_path || !out)
		return fail(PGX_E_ARG, "pgx_barcode_reads: null argument");
	return guard("pgx_barcode_reads", [&]() -> int {
		std::string text;
		std::unique_ptr<pgx_barcodes> res(new pgx_barcodes());
		bool opened;
		PGX_TRY(barcode_inputs(reads_path, barcodes_path, nullptr, text, res->bars, opened));
		PGX_TRY(barcode_run(text, res->bars, *res));
		*out = res.release();
		return 0;
	});
}

int64_t pgx_barcodes_count(const pgx_barcodes *b) { return b ? (int64_t)b->bars.size() : 0; }
const char *pgx_barcodes_name(const pgx_barcodes *b, int64_t i) { return b && i >= 0 && i < (int64_t)b->bars.size() ? b->bars[(size_t)i].name.c_str() : nullptr; }
const char *pgx_barcodes_letters(const pgx_barcodes *b, int64_t i) { return b && i >= 0 && i < (int64_t)b->bars.size() ? b->bars[(size_t)i].letters.c_str() : nullptr; }
int64_t pgx_barcodes_reads(const pgx_barcodes *b, int64_t i) { return b && i >= 0 && i < (int64_t)b->bars.size() ? (int64_t)b->recs[(size_t)i + 1] : -1; }
int64_t pgx_barcodes_sequences(const pgx_barcodes *b) { return b ? (int64_t)b->n_seq : 0; }
int64_t pgx_barcodes_no_barcode(const pgx_barcodes *b) { return b ? (int64_t)b->recs[0] : 0; }
int64_t pgx_barcodes_thrown_out(const pgx_barcodes *b) { return b ? (int64_t)b->recs[b->bars.size() + 1] : 0; }

int pgx_barcodes_take_reads(const pgx_barcodes *b, int64_t i, pgx_reads **out)
{
	if (out)
		*out = nullptr;
	PGX_TRY(require_device());
	if (!b || !out || i < -1 || i >= (int64_t)b->bars.size())
		return fail(PGX_E_ARG, "pgx_barcodes_take_reads: bad argument");
	return guard("pgx_barcodes_take_reads", [&]() -> int {
		const uint64_t s = b->slice[(size_t)(i + 1)], n = b->slice[(size_t)(i + 2)] - s;
		if (n >= kDeviceSplitLimit)
			return fail(PGX_E_LIMIT, "pgx_barcodes_take_reads: a FASTA of 4 GiB or more");
		// the slice moved to the front of a buffer of its own (the splitter reads aligned words), HBM to HBM
		DevBuf<uint8_t> d;
		PGX_TRY(d.alloc(n, 0, 32));
		if (n)
			PGX_HIP(hipMemcpy(d.data(), b->out.data() + s, n, hipMemcpyDeviceToDevice));
		std::unique_ptr<pgx_reads> rd;
		PGX_TRY(reads_from_resident_fasta_text(d.data(), n, rd));
		*out = rd.release();
		return 0;
	});
}

void pgx_barcodes_free(pgx_barcodes *b) { delete b; }
}
