// barcode — drop-in for `perl Barcode/barcode.pl -s reads.fas -b barcodes.txt -d dir` (barcode.pl:18-43): the script walks
// @ARGV itself, so the words are passed through.  A file that cannot be created in `dir` ends the script with `die $!`:
// status 2 here; an input the library refuses (no -d, a barcode line it will not guess at, ...): status 3, nothing written.
#include <cstdio>
#include "pangea_hip.h"

int main(int argc, char **argv)
{
	char *log = nullptr;
	const int rc = pgx_barcode_file(argc - 1, argv + 1, &log);
	if (log)
		fputs(log, stdout);
	pgx_free(log);
	if (rc < 0) {
		fprintf(stderr, "barcode: %s\n", pgx_last_error());
		return rc == PGX_E_IO ? 2 : 3;
	}
	return 0;
}
