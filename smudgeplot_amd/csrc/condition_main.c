/*******************************************************************************************
 *
 *  smg_condition -- trim and / or symmetrise a FastK k-mer table on the GPU and write the result as a
 *                   FastK table again (format F: stub + part files).
 *
 *  What `hetmers` / `extract_kmer_pairs` of the reference obtain by shelling out to FastK's
 *  Logex '<t>=A[e-]' and Symmex (PloidyPlot.c:1381-1414), as a stand-alone tool: the reference's
 *  executables accept its output as "trimmed and symmetric" and skip their own conditioning.
 *
 *  Usage: smg_condition [-v] [-T<int(4)>] [-e<int(4)>] [-t] [-s] <source>[.ktab] <target>[.ktab]
 *           -e: trim threshold (keep count >= e)          -t: trim only      -s: symmetrise only
 *         (default: both steps; a table that the reference's probe already finds trimmed / symmetric
 *          still goes through the requested steps -- they are idempotent)
 *
 *  The target gets the source's prefix-index width (ibyte) and number of parts.  No CPU fallback.
 *
 ********************************************************************************************/

#include "smg_cli.h"

int main(int argc, char *argv[])
{ int verbose = 0, nthreads = 4, ethresh = 4, only_trim = 0, only_symm = 0;
  int i, j;
  smg_ktab T;
  smg_table_view tv;
  smg_opts opts;
  uint64_t *keys = NULL; uint16_t *cnt = NULL;
  int64_t n = 0;
  int W = 0;
  char errbuf[512];

  Prog_Name = "smg_condition";
  j = 1;
  for (i = 1; i < argc; i++)
    if (argv[i][0] == '-')
      switch (argv[i][1])
      { case 'v': verbose = 1; break;
        case 't': only_trim = 1; break;
        case 's': only_symm = 1; break;
        case 'e': ethresh = arg_positive(argv[i], "Error-mer threshold"); break;
        case 'T': nthreads = arg_positive(argv[i], "Number of threads"); if (nthreads > 64) nthreads = 64; break;
        default:
          fprintf(stderr, "%s: -%c is an illegal option\n", Prog_Name, argv[i][1]);
          exit(1);
      }
    else
      argv[j++] = argv[i];
  if (j != 3 || (only_trim && only_symm))
    { fprintf(stderr, "\nUsage: %s [-v] [-T<int(4)>] [-e<int(4)>] [-t] [-s] <source>[.ktab] <target>[.ktab]\n", Prog_Name);
      fprintf(stderr, "\n      -e: keep the k-mers with count >= e\n      -t: trim only\n      -s: symmetrise only\n");
      exit(1);
    }
  Load_Threads = nthreads;
  load_or_die(argv[1], &T);
  smg_cli_table_view(&T, &tv);
  memset(&opts, 0, sizeof(opts));
  { const char *g = getenv("SMUDGEPLOT_GPU"); opts.device = g ? atoi(g) : 0; }
  opts.ethresh = ethresh;
  opts.condition = (only_symm ? 0 : SMG_COND_TRIM) | (only_trim ? 0 : SMG_COND_SYMM);
  errbuf[0] = 0;
  if (smg_condition_table(&tv, &opts, &keys, &cnt, &n, &W, errbuf, sizeof(errbuf)) != SMG_OK)
    { fprintf(stderr, "%s: %s\n", Prog_Name, errbuf[0] ? errbuf : "GPU engine failed"); exit(1); }
  if (verbose)
    fprintf(stderr, "  %lld -> %lld k-mers (k=%d%s%s)\n", (long long) T.nels, (long long) n, T.kmer,
            only_symm ? "" : ", trimmed", only_trim ? "" : ", symmetrised");

  /* ---- write format F: the target gets the source's prefix-index width and number of parts ---------------- */
  if (smg_cli_write_ktab(argv[2], T.kmer, T.ibyte, T.nparts, only_symm ? T.minval : (T.minval > ethresh ? T.minval : ethresh),
                         keys, cnt, n, W))
    exit(1);
  smg_free(keys); smg_free(cnt);
  smg_ktab_free(&T);
  exit(0);
}
