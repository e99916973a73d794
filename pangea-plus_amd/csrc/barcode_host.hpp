// Barcode/barcode.pl: the parts that stay on the host -- the barcode file, and the file's last record, which the script
// processes with the line count of the record before it (tests/barcode_rule.py spells the rule out).  No HIP in here: a
// stand-alone program (tests/host/barcode_host_test.cpp) runs this file under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/pangea_hip.h"

namespace pgx {

constexpr size_t kBcMaxBars = 2048, kBcMaxLetters = 64;

struct BcBar {
	std::string name, letters; // letters upper-cased (barcode.pl:89)
};

inline bool bc_space(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); } // Perl's \s on bytes

// barcode.pl:84-93, one `name TAB letters` per line.  0, or PGX_E_ARG / PGX_E_LIMIT with the reason in `why`: a line with
// no tab, an empty name, empty letters or letters outside [A-Za-z] (the script interpolates them into a regex), a name with
// '/' or NUL or one used twice (the script would write elsewhere, or twice into one file).
inline int bc_parse_barcodes(const std::string &text, std::vector<BcBar> &out, std::string &why)
{
	out.clear();
	std::unordered_set<std::string> seen;
	size_t line_no = 0;
	for (size_t s = 0; s < text.size();) {
		const size_t nl = text.find('\n', s);
		const size_t e = nl == std::string::npos ? text.size() : nl + 1;
		line_no++;
		auto bad = [&](const char *what) {
			why = "barcode file line " + std::to_string(line_no) + ": " + what;
			return (int)PGX_E_ARG;
		};
		const void *t = memchr(text.data() + s, '\t', e - s);
		if (!t)
			return bad("no tab");
		const size_t tab = (size_t)((const char *)t - text.data());
		size_t end = e;
		while (end > s && bc_space((unsigned char)text[end - 1])) // s/\s+$//
			end--;
		BcBar b;
		b.name.assign(text, s, tab - s);
		if (end > tab + 1)
			b.letters.assign(text, tab + 1, end - (tab + 1));
		if (b.name.empty())
			return bad("empty name");
		if (b.letters.empty())
			return bad("no letters");
		for (char &c : b.letters) {
			if (c >= 'a' && c <= 'z')
				c = (char)(c - 'a' + 'A');
			if (c < 'A' || c > 'Z')
				return bad("letters outside A-Z");
		}
		if (b.name.find('/') != std::string::npos || b.name.find('\0') != std::string::npos)
			return bad("'/' or NUL in the name");
		if (!seen.insert(b.name).second)
			return bad("name used twice");
		if (b.letters.size() > kBcMaxLetters) {
			why = "barcode file line " + std::to_string(line_no) + ": more than 64 letters";
			return PGX_E_LIMIT;
		}
		out.push_back(std::move(b));
		s = e;
	}
	if (out.size() > kBcMaxBars) {
		why = "more than 2048 barcodes";
		return PGX_E_LIMIT;
	}
	return 0;
}

struct BcLine {
	uint64_t off, len; // with its line end
};

// The stored lines of the file's last record (header first; lines that are exactly "\n" are not stored, :109) and the
// number of stored lines of the record before it (0 when there is none): a walk back from the end of the text.
// false: the text holds no header line.
inline bool bc_tail_records(const char *text, uint64_t n, std::vector<BcLine> &last, uint64_t &stale)
{
	last.clear();
	stale = 0;
	int headers = 0;
	uint64_t end = n;
	while (end > 0) {
		const void *q = end > 1 ? memrchr(text, '\n', end - 1) : nullptr;
		const uint64_t s = q ? (uint64_t)((const char *)q - text) + 1 : 0;
		const uint64_t len = end - s;
		const bool header = memchr(text + s, '>', len) != nullptr;
		const bool stored = header || !(len == 1 && text[s] == '\n');
		if (headers == 0) {
			if (stored)
				last.push_back(BcLine{ s, len });
		} else if (stored) {
			stale++;
		}
		if (header && ++headers == 2)
			break;
		end = s;
	}
	std::reverse(last.begin(), last.end());
	if (headers < 2)
		stale = 0; // (lines before the first header are refused elsewhere)
	return headers > 0;
}

// What the script decides for one record and what it then writes, as byte ranges of the input
struct BcFate {
	int status = 0;        // 0, or PGX_E_REFHANG: the script never ends on this record
	int bar = -1;          // -1: no barcode
	long long bases = 0;
	bool kept = false;     // bar >= 0 and bases >= 100
	uint64_t body_begin = 0, body_end = 0; // the bytes written behind the header (all of the record for bar == -1)
	uint64_t size = 0;     // bytes written
	uint32_t pushed = 0;   // lines pushed onto the barcode's list (:232-254)
};

inline long long bc_index(const char *text, const BcLine &l, const std::string &w)
{
	if (w.size() > l.len)
		return -1;
	const void *p = memmem(text + l.off, l.len, w.data(), w.size());
	return p ? (long long)((const char *)p - (text + l.off)) : -1;
}

// find_and_store_barcode (:164-255) on the LAST record: `stale` is the global $storeSize return_bases reads (:263).
inline BcFate bc_last_record(const char *text, const std::vector<BcLine> &lines, const std::vector<BcBar> &bars, uint64_t stale)
{
	BcFate f;
	const uint64_t S = lines.size(), G = stale;
	uint64_t place = 0;
	auto bases_of = [&](int a, uint64_t pl) { // return_bases
		long long v = 60 - (bc_index(text, lines[pl], bars[a].letters) + (long long)bars[a].letters.size());
		for (uint64_t k = pl + 1; k < G && k < S; k++)
			v += (long long)lines[k].len;
		return v;
	};
	for (uint64_t b = 1; b < S; b++) {
		const BcLine &l = lines[b];
		bool hit = false;
		for (size_t a = 0; a < bars.size() && !hit; a++) { // :185-194, $first stays 1
			const std::string &w = bars[a].letters;
			if (w.size() <= l.len && !memcmp(text + l.off, w.data(), w.size())) {
				hit = true;
				f.bar = (int)a;
				place = 1;
				f.bases = bases_of((int)a, 1);
				const uint64_t nb = std::max<uint64_t>(2, G);
				if (nb + 1 <= b) { // $b is set back to or before this line
					f.status = PGX_E_REFHANG;
					return f;
				}
				b = nb;
			}
		}
		if (f.bar == -1) {
			for (size_t a = 0; a < bars.size(); a++) { // :199-208
				if (bc_index(text, l, bars[a].letters) >= 0) {
					f.bar = (int)a;
					place = b;
					f.bases = bases_of((int)a, b);
					b = std::max(b + 1, G);
					break;
				}
			}
		}
	}
	// `while($temp = shift(@storedLines))` ends at a false line: a last line "0" with no line end
	uint64_t n_shift = S;
	if (S && lines[S - 1].len == 1 && text[lines[S - 1].off] == '0')
		n_shift = S - 1;
	if (S == 0) { // (:116 on an empty file: $thisBar is still 0, $bases 0)
		f.bar = 0;
		return f;
	}
	const uint64_t rec_end = n_shift ? lines[n_shift - 1].off + lines[n_shift - 1].len : lines[0].off;
	if (f.bar == -1) {
		f.body_begin = lines[0].off;
		f.body_end = rec_end;
		for (uint64_t k = 0; k < n_shift; k++)
			f.size += lines[k].len;
		f.size += 1;
		return f;
	}
	if (f.bases < 100)
		return f;
	f.kept = true;
	const std::string &w = bars[f.bar].letters;
	f.size = lines[0].len + bars[f.bar].name.size() + 1 + 1; // '>' name '_' header[1:] ... "\n"
	f.pushed = 2;
	f.body_begin = f.body_end = rec_end;
	if (n_shift == 0) { // (the header itself was the false line: cannot be, a header holds '>')
		return f;
	}
	if (place < n_shift) {
		const BcLine &l = lines[place];
		const uint64_t cut = std::min<uint64_t>((uint64_t)(bc_index(text, l, w) + (long long)w.size()), l.len);
		f.body_begin = l.off + cut;
		f.size += l.len - cut;
		f.pushed++;
		for (uint64_t k = place + 1; k < n_shift; k++) {
			f.size += lines[k].len;
			f.pushed++;
		}
	}
	return f;
}

} // namespace pgx
