// The locus-key rule of the seed stage's read ordering (pangea-plus_amd/csrc/read_order.hpp), compiled for the host: the
// bin geometry at the database sizes that matter, and the strand / probe choice against a brute-force restatement on
// hand-made and random bucket contents.  The kernel compiles the same header.
#include "../../pangea-plus_amd/csrc/read_order.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

using namespace pgx;

static int failures = 0;
#define CHECK(cond, ...)                                                                                                \
	do {                                                                                                            \
		if (!(cond)) {                                                                                          \
			failures++;                                                                                     \
			printf("DIFFERENT %s:%d: %s: ", __FILE__, __LINE__, #cond);                                     \
			printf(__VA_ARGS__);                                                                            \
			printf("\n");                                                                                   \
		}                                                                                                       \
	} while (0)

// an index as a map from k-mer to its position-sorted postings
struct MapIndex {
	std::vector<uint32_t> postings;
	std::map<uint32_t, OrderRange> buckets;
	mutable int ranges = 0, firsts = 0;
	void add(uint32_t kmer, std::vector<uint32_t> pos)
	{
		buckets[kmer] = OrderRange{ (uint32_t)postings.size(), (uint32_t)pos.size() };
		postings.insert(postings.end(), pos.begin(), pos.end());
	}
	OrderRange range(uint32_t kmer) const
	{
		ranges++;
		auto it = buckets.find(kmer);
		return it == buckets.end() ? OrderRange{ 0xDEAD0000u, 0u } : it->second; // (lo of an empty bucket must never be followed)
	}
	uint32_t first(uint32_t lo) const
	{
		firsts++;
		if (lo >= postings.size()) {
			printf("DIFFERENT first(%u) outside the postings\n", lo);
			failures++;
			return 0;
		}
		return postings[lo];
	}
};

// the rule once more, as a table: all four buckets looked up, strand by (first count, second count), forward on a full tie
static uint32_t brute(const MapIndex &ix, const uint32_t kmer[2][2], const bool usable[2][2], int shift, uint32_t last_bin)
{
	uint32_t cnt[2][2], lo[2][2];
	for (int s = 0; s < 2; s++)
		for (int j = 0; j < 2; j++) {
			auto it = usable[s][j] ? ix.buckets.find(kmer[s][j]) : ix.buckets.end();
			cnt[s][j] = it == ix.buckets.end() ? 0 : it->second.cnt;
			lo[s][j] = it == ix.buckets.end() ? 0 : it->second.lo;
		}
	int strand;
	if (cnt[0][0] != cnt[1][0])
		strand = cnt[1][0] > cnt[0][0];
	else
		strand = cnt[1][1] > cnt[0][1];
	int probe;
	if (cnt[strand][0])
		probe = 0;
	else if (cnt[strand][1] && cnt[0][0] == 0 && cnt[1][0] == 0)
		probe = 1;
	else
		return last_bin;
	const uint64_t bin = (uint64_t)ix.postings[lo[strand][probe]] >> shift;
	return bin < last_bin ? (uint32_t)bin : last_bin;
}

static void test_geometry()
{
	const int64_t sizes[] = { 1, 1ll << 20, 1000000000ll, 3000000000ll, (1ll << 32) - 1 };
	const int want_shift[] = { 0, 5, 14, 16, 17 };
	for (int i = 0; i < 5; i++) {
		const int64_t n = sizes[i];
		const int s = read_order_shift(n);
		const uint32_t last = read_order_last_bin(n);
		const int bits = read_order_key_bits(n);
		// brute force: the smallest shift whose position bins plus the no-key bin are at most 65 536
		int bs = 0;
		while ((((n - 1) >> bs) + 1) + 1 > 65536)
			bs++;
		CHECK(s == bs && s == want_shift[i], "n_bases %lld: shift %d, brute force %d, expected %d", (long long)n, s, bs, want_shift[i]);
		CHECK(last == (uint32_t)((n - 1) >> s) + 1 && last <= 65535, "n_bases %lld: last bin %u", (long long)n, last);
		CHECK(((uint64_t)(n - 1) >> s) < last, "n_bases %lld: the top position's bin %llu is no position bin", (long long)n,
		      (unsigned long long)((uint64_t)(n - 1) >> s));
		CHECK((1ull << bits) > last && (bits == 1 || (1ull << (bits - 1)) <= last) && bits <= 16, "n_bases %lld: %d key bits for last bin %u",
		      (long long)n, bits, last);
		if (s > 0) // one shift less would not fit
			CHECK(((n - 1) >> (s - 1)) + 2 > 65536, "n_bases %lld: shift %d is not the smallest", (long long)n, s);
		// the top position through the rule itself
		MapIndex ix;
		ix.add(7u, { (uint32_t)(n - 1) });
		const uint32_t kmer[2][2] = { { 7u, 0u }, { 1u, 2u } };
		const bool usable[2][2] = { { true, false }, { true, false } };
		const uint32_t k = read_order_key(ix, kmer, usable, s, last);
		CHECK(k < last && k == (uint32_t)((uint64_t)(n - 1) >> s), "n_bases %lld: key %u of the top position", (long long)n, k);
	}
	printf("geometry ok\n");
}

static void test_hand_made()
{
	const int shift = 4;
	const uint32_t last = 1000;
	MapIndex ix;
	ix.add(100u, { 320, 640, 1600 }); // a real locus: three relatives
	ix.add(200u, { 4800 });           // a chance bucket
	ix.add(300u, { 8000 });
	ix.add(400u, { 9600, 9700 });
	ix.add(500u, { 0xFFFFFFF0u });    // a posting beyond every bin
	struct Case {
		const char *what;
		uint32_t kmer[2][2];
		bool usable[2][2];
		uint32_t want;
		int ranges;
	} cases[] = {
		{ "forward alone", { { 100u, 1u }, { 2u, 3u } }, { { true, true }, { true, true } }, 320 >> 4, 2 },
		{ "reverse alone", { { 2u, 3u }, { 100u, 1u } }, { { true, true }, { true, true } }, 320 >> 4, 2 },
		{ "fuller reverse beats a chance forward", { { 200u, 1u }, { 100u, 2u } }, { { true, true }, { true, true } }, 320 >> 4, 2 },
		{ "fuller forward beats a chance reverse", { { 400u, 1u }, { 300u, 2u } }, { { true, true }, { true, true } }, 9600 >> 4, 2 },
		{ "tie, second probe of the reverse strand decides", { { 200u, 1u }, { 300u, 400u } }, { { true, true }, { true, true } }, 8000 >> 4, 4 },
		{ "tie, second probe of the forward strand decides", { { 200u, 100u }, { 300u, 400u } }, { { true, true }, { true, true } }, 4800 >> 4, 4 },
		{ "full tie: forward", { { 200u, 1u }, { 300u, 2u } }, { { true, true }, { true, true } }, 4800 >> 4, 4 },
		{ "first probes empty: the second of the reverse strand", { { 1u, 2u }, { 3u, 100u } }, { { true, true }, { true, true } }, 320 >> 4, 4 },
		{ "first probes empty: the fuller second", { { 1u, 200u }, { 3u, 400u } }, { { true, true }, { true, true } }, 9600 >> 4, 4 },
		{ "nothing anywhere", { { 1u, 2u }, { 3u, 4u } }, { { true, true }, { true, true } }, last, 4 },
		{ "a read of 16 to 28 bases: no second probe", { { 1u, 100u }, { 3u, 100u } }, { { true, false }, { true, false } }, last, 2 },
		{ "a read under 16 bases", { { 100u, 100u }, { 100u, 100u } }, { { false, false }, { false, false } }, last, 0 },
		{ "ambiguity in the forward first probe", { { 100u, 1u }, { 200u, 2u } }, { { false, true }, { true, true } }, 4800 >> 4, 1 },
		{ "a posting beyond the bins", { { 500u, 1u }, { 2u, 3u } }, { { true, true }, { true, true } }, last, 2 },
	};
	for (const Case &c : cases) {
		ix.ranges = ix.firsts = 0;
		const uint32_t got = read_order_key(ix, c.kmer, c.usable, shift, last);
		CHECK(got == c.want, "%s: key %u, expected %u", c.what, got, c.want);
		CHECK(ix.ranges == c.ranges && ix.firsts == (got == last && c.kmer[0][0] != 500u ? 0 : 1), "%s: %d bucket look-ups (expected %d), %d posting look-ups",
		      c.what, ix.ranges, c.ranges, ix.firsts);
		const uint32_t b = brute(ix, c.kmer, c.usable, shift, last);
		CHECK(got == b, "%s: key %u, brute force %u", c.what, got, b);
	}
	printf("hand-made buckets ok\n");
}

static void test_random()
{
	std::mt19937_64 rng(12345);
	for (int round = 0; round < 200; round++) {
		const int64_t n_bases = round % 2 ? 5000000 : (1ll << 32) - 1;
		const int shift = read_order_shift(n_bases);
		const uint32_t last = read_order_last_bin(n_bases);
		MapIndex ix;
		for (uint32_t k = 0; k < 12; k++) {
			if (rng() % 3 == 0)
				continue; // an empty bucket
			std::vector<uint32_t> pos(1 + rng() % 3);
			uint32_t p = (uint32_t)(rng() % (uint64_t)n_bases);
			for (auto &x : pos) {
				x = p;
				p = (uint32_t)std::min<uint64_t>((uint64_t)p + rng() % 1000, (uint64_t)n_bases - 1);
			}
			ix.add(k, pos);
		}
		for (int t = 0; t < 200; t++) {
			uint32_t kmer[2][2];
			bool usable[2][2];
			for (int s = 0; s < 2; s++)
				for (int j = 0; j < 2; j++) {
					kmer[s][j] = (uint32_t)(rng() % 12);
					usable[s][j] = rng() % 8 != 0;
				}
			const uint32_t got = read_order_key(ix, kmer, usable, shift, last), b = brute(ix, kmer, usable, shift, last);
			CHECK(got == b && got <= last, "round %d: key %u, brute force %u (last bin %u)", round, got, b, last);
			if (failures > 20)
				return;
		}
	}
	printf("random buckets ok\n");
}

int main()
{
	test_geometry();
	test_hand_made();
	test_random();
	if (failures) {
		printf("%d checks DIFFERENT\n", failures);
		return 1;
	}
	printf("read order key: all ok\n");
	return 0;
}
