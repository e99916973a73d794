/* oracle/ — TEST INFRASTRUCTURE ONLY (see o_common.h).
 *
 * Checks the cut the device makes in spec S3d (csrc/dust.hip) against the DEFINITION restated in o_dust.c.
 * The device's first pass (k_dust_scan) keeps, per triplet position, what the published algorithm (Morgulis et al. 2006)
 * keeps: the pair count r_w of the window of the last at most 62 triplets, and L = min(window size, length of the longest
 * suffix in which no triplet value occurs more than 4 times); a position PASSES when 10 r_w > 20 L.  A letter that is no
 * base empties the window.  A read is listed when a position passes, with the first and the last such position, and the
 * second pass (k_dust_perfect) runs the definition on the listed reads alone, and only on triplet intervals [a, b] with
 * a >= first - 61 and b <= last.  Here the first pass is stated plainly, by brute force over the window (none of the
 * device's incremental bookkeeping), and the program fails when
 *   - a read with a masked base (definition) is not listed, or
 *   - the definition restricted to those intervals gives a mask other than o_dust_mask's.
 * Reads: uniform, biased, with noisy repeats of unit 1-6 up to 200 bases long, with an N; every tenth up to 1 500 bases;
 * and the reads of a file, one per line (tests/dust_rule.py: crafted_reads).
 * usage: fuzz_dust [reads [file]]     (tests/test_oracle_classify.py runs it with 60 000 and the crafted reads)
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
void o_dust_mask(const uint8_t *base, int32_t len, uint8_t *mask);
#define MAXLEN 1600
#define MAXT 62

static int triplets(const uint8_t *base, int len, int *trip)
{
	const int nt = len - 2;
	for (int i = 0; i < nt; i++)
		trip[i] = (base[i] < 4 && base[i + 1] < 4 && base[i + 2] < 4) ? base[i] * 16 + base[i + 1] * 4 + base[i + 2] : -1;
	return nt > 0 ? nt : 0;
}

/* the first pass: 1 when a position passes; *first, *last = the first and the last one */
static int first_pass(const int *trip, int nt, int *first, int *last)
{
	int clean = 0; /* triplets since the last one that holds no-base letters */
	*first = *last = -1;
	for (int b = 0; b < nt; b++) {
		if (trip[b] < 0) {
			clean = 0;
			continue;
		}
		clean++;
		const int size = clean < MAXT ? clean : MAXT;
		int cnt[64] = { 0 }, rw = 0;
		for (int k = b - size + 1; k <= b; k++)
			rw += cnt[trip[k]]++;
		int L = 0;
		memset(cnt, 0, sizeof cnt);
		for (int k = b; k > b - size && cnt[trip[k]] < 4; k--) {
			cnt[trip[k]]++;
			L++;
		}
		if (10 * rw > 20 * L) {
			if (*first < 0)
				*first = b;
			*last = b;
		}
	}
	return *first >= 0;
}

/* the definition (o_dust.c's header) on the intervals [a, b] with a_lo <= a and b <= b_hi only; scores as exact fractions */
static int better(long r1, long q1, long r2, long q2) /* r1 / q1 > r2 / q2; q = 0: no score, below every score */
{
	if (q1 == 0)
		return 0;
	if (q2 == 0)
		return 1;
	return r1 * q2 > r2 * q1;
}
static void mask_in_range(const int *trip, int nt, int len, int a_lo, int b_hi, uint8_t *mask)
{
	static long br[2][MAXT + 1], bq[2][MAXT + 1]; /* best score of any sub-interval of [a, a + k], rows a and a + 1 */
	memset(mask, 0, (size_t)len);
	memset(bq, 0, sizeof bq);
	memset(br, 0, sizeof br);
	if (b_hi > nt - 1)
		b_hi = nt - 1;
	if (a_lo < 0)
		a_lo = 0;
	for (int a = b_hi; a >= a_lo; a--) {
		long *row_r = br[a & 1], *row_q = bq[a & 1], *low_r = br[(a + 1) & 1], *low_q = bq[(a + 1) & 1];
		int cnt[64] = { 0 }, k = 0;
		long r = 0, left_r = 0, left_q = 0;
		for (; a + k <= b_hi && k < MAXT && trip[a + k] >= 0; k++) {
			r += cnt[trip[a + k]]++;
			long sub_r = left_r, sub_q = left_q;
			if (k > 0 && better(low_r[k - 1], low_q[k - 1], sub_r, sub_q))
				sub_r = low_r[k - 1], sub_q = low_q[k - 1];
			if (k > 0 && 10 * r > 20 * (long)k && !better(sub_r, sub_q, r, k))
				memset(mask + a, 1, (size_t)k + 3);
			if (better(r, k, sub_r, sub_q))
				sub_r = r, sub_q = k;
			row_r[k] = left_r = sub_r;
			row_q[k] = left_q = sub_q;
		}
		for (; k <= MAXT; k++)
			row_r[k] = row_q[k] = 0;
	}
}

static uint64_t sd = 88172645463325252ull;
static uint32_t rnd(void) { sd ^= sd << 13; sd ^= sd >> 7; sd ^= sd << 17; return (uint32_t)(sd >> 11); }

static long n_reads, n_masked, n_listed, n_unlisted, n_range, n_uniform, n_uniform_masked, n_uniform_listed, n_long;
static void check(const uint8_t *b, int len, int uniform, const char *what)
{
	static uint8_t m[MAXLEN], m2[MAXLEN];
	static int trip[MAXLEN];
	o_dust_mask(b, len, m);
	int any = 0, first, last;
	for (int i = 0; i < len; i++)
		any |= m[i];
	const int nt = triplets(b, len, trip);
	const int listed = first_pass(trip, nt, &first, &last);
	n_reads++;
	n_masked += any;
	n_listed += listed;
	n_long += len > 512;
	if (uniform) {
		n_uniform++;
		n_uniform_masked += any;
		n_uniform_listed += listed;
	}
	int bad = 0;
	if (any && !listed) {
		bad = 1;
		n_unlisted++;
	} else if (listed) {
		mask_in_range(trip, nt, len, first - (MAXT - 1), last, m2);
		if (memcmp(m, m2, (size_t)len) != 0) {
			bad = 2;
			n_range++;
		}
	}
	if (bad && n_unlisted + n_range <= 5) {
		printf("%s (%s) len %d first %d last %d: ", bad == 1 ? "COUNTEREXAMPLE not listed" : "COUNTEREXAMPLE range", what, len, first, last);
		for (int i = 0; i < len; i++)
			putchar("ACGTN"[b[i]]);
		putchar('\n');
	}
}

int main(int argc, char **argv)
{
	const long n = argc > 1 ? atol(argv[1]) : 100000;
	static uint8_t b[MAXLEN];
	for (long it = 0; it < n; it++) {
		int kind = rnd() % 6;
		int len = kind == 0 ? 150 : 20 + rnd() % 300;
		if (it % 10 == 9)
			len = 20 + rnd() % 1481;
		int bias = rnd() % 4;
		for (int i = 0; i < len; i++) {
			uint32_t x = rnd();
			b[i] = (kind == 5 && bias) ? ((x % 10) < 8 ? (x >> 8) % 2 * 3 : (x >> 8) & 3) : (x & 3); /* AT-rich */
		}
		if (kind >= 2 && kind <= 4) { /* repeats with noise */
			int nrep = 1 + rnd() % 3;
			for (int r = 0; r < nrep; r++) {
				int unit = 1 + rnd() % 6, ul[6], s0 = rnd() % len, rl = 4 + rnd() % (r == 0 ? 197 : 60), noise = rnd() % 12;
				for (int u = 0; u < unit; u++) ul[u] = rnd() & 3;
				for (int i = s0; i < s0 + rl && i < len; i++) {
					b[i] = ul[(i - s0) % unit];
					if (noise && rnd() % 12 < (uint32_t)noise / 3) b[i] = rnd() & 3;
				}
			}
		}
		if (kind == 4 && rnd() % 3 == 0) b[rnd() % len] = 4; /* an N */
		check(b, len, kind == 0 && len == 150, "generated");
	}
	long n_file = 0;
	if (argc > 2) {
		FILE *f = fopen(argv[2], "r");
		if (!f) {
			fprintf(stderr, "cannot open %s\n", argv[2]);
			return 2;
		}
		static char line[MAXLEN + 8];
		while (fgets(line, sizeof line, f)) {
			int len = 0;
			for (const char *p = line; *p && *p != '\n' && *p != '\r'; p++) {
				const char u = (char)(*p & 0xDF);
				b[len++] = u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : (u == 'T' || u == 'U') ? 3 : 4;
			}
			if (len > 0 && len < MAXLEN) {
				check(b, len, 0, "file");
				n_file++;
			}
		}
		fclose(f);
	}
	printf("reads %ld (from the file %ld, above 512 bases %ld) masked %ld listed %ld counterexamples %ld range mismatches %ld | uniform 150: %ld masked %ld listed %ld\n",
	       n_reads, n_file, n_long, n_masked, n_listed, n_unlisted, n_range, n_uniform, n_uniform_masked, n_uniform_listed);
	return n_unlisted != 0 || n_range != 0;
}
