// unclassified_selector — drop-in for `perl Unclas_Sel/unclassified_selector.pl -m table.tsv -s reads.fas -o out.fas
// [-t PCT] [-e LN_EVALUE] [-b BITS]` (unclassified_selector.pl:21-59): the script walks @ARGV itself, so the words are
// passed through.  An -o file that cannot be created ends the script with `die $!` (:123): status 2 here.
#include <cstdio>
#include "pangea_hip.h"

int main(int argc, char **argv)
{
	char *log = nullptr;
	const int rc = pgx_unclas_file(argc - 1, argv + 1, &log);
	if (log)
		fputs(log, stdout);
	pgx_free(log);
	if (rc < 0) {
		fprintf(stderr, "unclassified_selector: %s\n", pgx_last_error());
		return rc == PGX_E_IO ? 2 : 3;
	}
	return 0;
}
