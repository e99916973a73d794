// The locus key of a read: where in the database the seed stage will most likely look for it.  A search sorts its reads by
// this key and walks them in that order, so that reads of one database region run next to one another and the region's
// database words and block records are L2 hits for all but the first of them (classify.hip: order_reads).
// Free of HIP: the kernel (classify.hip: k_read_order_keys) and a stand-alone host test (tests/host/read_order_test.cpp)
// compile the same rule.  A wrong key is never an error: it only costs that read its locality.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PGX_HD __host__ __device__
#else
#define PGX_HD
#endif

namespace pgx {

// probe offsets inside a strand: the seed kernel's first two probes (stride 13), so a read of 16 bases has the first, one of
// 29 both
constexpr int kOrderProbe0 = 0, kOrderProbe1 = 13;
constexpr int kOrderProbeLen = 16;
// position bins and the bin of reads without a key together: 16 key bits, two 8-bit radix passes
constexpr uint32_t kOrderMaxBins = 65536;

// bin = posting >> shift: the smallest shift with which the bins of positions 0 .. n_bases - 1 and one more bin (reads without a
// key: the last) are at most 65 536.  1 Gbp: shift 14, bins of 16 kbases; databases under 64 kbases: shift 0
PGX_HD inline int read_order_shift(int64_t n_bases)
{
	const int64_t top = n_bases > 0 ? n_bases - 1 : 0;
	int s = 0;
	while ((top >> s) + 2 > (int64_t)kOrderMaxBins)
		s++;
	return s;
}
// the bin of reads without a usable probe (shorter than 16 bases, no posting, ambiguity letters in the probes); also the number
// of position bins
PGX_HD inline uint32_t read_order_last_bin(int64_t n_bases)
{
	const int64_t top = n_bases > 0 ? n_bases - 1 : 0;
	return (uint32_t)(top >> read_order_shift(n_bases)) + 1u;
}
// key bits the sort has to look at
PGX_HD inline int read_order_key_bits(int64_t n_bases)
{
	const uint32_t last = read_order_last_bin(n_bases);
	int b = 1;
	while (b < 32 && (last >> b) != 0)
		b++;
	return b;
}

struct OrderRange {
	uint32_t lo, cnt; // first posting of a bucket, postings in it
};

// kmer[s][j] / usable[s][j]: probe j (offsets kOrderProbe0, kOrderProbe1) of strand s (0 forward, 1 reverse complement), and
// whether it exists and is free of ambiguity letters.  Index: range(kmer) = the k-mer's bucket, first(lo) = the posting at
// index lo (postings are position-sorted inside a bucket, so this is the lowest position of the bucket).
// The rule: the first probes of both strands are looked up together.  The strand with the FULLER bucket gives the key: a read
// lies on one strand only, the other strand's probe finds a bucket by chance (at 1 Gbp in 2^32 buckets with probability
// 0.21, and then one posting, where the relatives of a real locus give many).  Equally full -- most often both empty, a
// substitution in the first 16 bases -- the second probes are looked up and decide in the same way: between the strands
// where the first probes tie above zero, and as the source of the key where the first probes found nothing.  Nothing
// anywhere: the last bin.  Lines per read: two bucket lines and one posting line, two more bucket lines for the ties.
template <class Index>
PGX_HD inline uint32_t read_order_key(const Index &ix, const uint32_t kmer[2][2], const bool usable[2][2], int shift, uint32_t last_bin)
{
	const OrderRange none = { 0u, 0u };
	const OrderRange f0 = usable[0][0] ? ix.range(kmer[0][0]) : none, r0 = usable[1][0] ? ix.range(kmer[1][0]) : none;
	uint32_t lo;
	if (f0.cnt != r0.cnt)
		lo = r0.cnt > f0.cnt ? r0.lo : f0.lo;
	else {
		const OrderRange f1 = usable[0][1] ? ix.range(kmer[0][1]) : none, r1 = usable[1][1] ? ix.range(kmer[1][1]) : none;
		const bool rev = r1.cnt > f1.cnt;
		if (f0.cnt)
			lo = rev ? r0.lo : f0.lo;
		else if (f1.cnt | r1.cnt)
			lo = rev ? r1.lo : f1.lo;
		else
			return last_bin;
	}
	const uint32_t bin = ix.first(lo) >> shift;
	return bin < last_bin ? bin : last_bin;
}

} // namespace pgx
