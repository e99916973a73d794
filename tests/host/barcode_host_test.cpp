// The host-side text code of the barcode demultiplexer (pangea-plus_amd/csrc/barcode_host.hpp: the barcode file, the walk
// back over the file's last two records, the last record's own rule) under AddressSanitizer + UndefinedBehaviorSanitizer.
// usage: barcode_host_asan GOLDEN_DIR -- one line per case directory that holds both inputs:
//   <case> parse=<status> bars=<n> last=<status> bar=<index> kept=<0|1> bases=<n> lines=<stored lines> stale=<n>
// tests/test_barcode_host.py compares the lines with tests/barcode_rule.py.
#include <cstdio>
#include <filesystem>
#include <fstream>
#include <iterator>
#include <set>

#include "../../pangea-plus_amd/csrc/barcode_host.hpp"

static bool slurp(const std::filesystem::path &p, std::string &out)
{
	std::ifstream f(p, std::ios::binary);
	if (!f)
		return false;
	out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
	return true;
}

int main(int argc, char **argv)
{
	if (argc != 2) {
		fprintf(stderr, "usage: %s GOLDEN_DIR\n", argv[0]);
		return 2;
	}
	std::set<std::filesystem::path> cases;
	for (const auto &e : std::filesystem::directory_iterator(argv[1]))
		if (e.is_directory())
			cases.insert(e.path());
	for (const auto &dir : cases) {
		std::string btext, text, why;
		if (!slurp(dir / "barcodes.txt", btext) || !slurp(dir / "reads.fas", text))
			continue;
		std::vector<pgx::BcBar> bars;
		const int prc = pgx::bc_parse_barcodes(btext, bars, why);
		printf("%s parse=%d bars=%zu", dir.filename().c_str(), prc, bars.size());
		if (prc == 0) {
			// (an exact-size copy, so that a read past the text is a read past the allocation)
			std::vector<char> exact(text.begin(), text.end());
			std::vector<pgx::BcLine> last;
			uint64_t stale = 0;
			const bool any = pgx::bc_tail_records(exact.data(), exact.size(), last, stale);
			const pgx::BcFate f = pgx::bc_last_record(exact.data(), last, bars, stale);
			printf(" any=%d last=%d bar=%d kept=%d bases=%lld lines=%zu stale=%llu", (int)any, f.status, f.bar, (int)f.kept, f.bases, last.size(),
			       (unsigned long long)stale);
		}
		printf("\n");
	}
	return 0;
}
