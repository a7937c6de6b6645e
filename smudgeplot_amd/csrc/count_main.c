/*******************************************************************************************
 *
 *  smg_count -- count the canonical k-mers of FASTA / FASTQ reads on the GPU and write them as a FastK
 *               k-mer table (format F: stub + one hidden part file, 3-byte prefix index), plus the
 *               k-mer count histogram that `smudgeplot cutoff` reads.
 *
 *  The step in front of `hetmers`: where a smudgeplot run starts from reads, this stands in for FastK.
 *
 *  Usage: smg_count [-v] [-T<int(4)>] [-k<int(31)>] [-t<int(4)>] [-p<int(0)>] [-H] [-o<output>] <reads> ...
 *           -k: k-mer length, 13 .. 128          -t: keep the k-mers with count >= t
 *           -H: also write <output>.hist.txt     -T: reader threads (one input file each, at most 16)
 *           -o: root name of the table; default is the root of the first input
 *           -p: key ranges to count in: 0 as many as the data need, 1 one pass, 2 .. 4096 that many
 *
 *  SMUDGEPLOT_GPU picks the device.  No CPU fallback.  A failed run leaves no table files behind.
 *
 ********************************************************************************************/

#include "smg_cli.h"
#include "smg_count.h"

static void usage(void)
{ fprintf(stderr, "\nUsage: %s [-v] [-T<int(4)>] [-k<int(31)>] [-t<int(4)>] [-p<int(0)>] [-H] [-o<output>] <reads> ...\n", Prog_Name);
  fprintf(stderr, "\n");
  fprintf(stderr, "      -k: k-mer length (13 .. %d)\n", SMG_MAX_KMER);
  fprintf(stderr, "      -t: keep the k-mers that occur at least t times\n");
  fprintf(stderr, "      -p: count in this many ranges of canonical k-mers (0 .. %d): 0 as many as the data need, 1 one pass\n", SMG_COUNT_BINS);
  fprintf(stderr, "      -H: write the k-mer count histogram to <output>.hist.txt\n");
  fprintf(stderr, "      -o: root name for the output table\n");
  fprintf(stderr, "            default is root of the first <reads> argument\n");
  fprintf(stderr, "      -v: verbose mode\n");
  fprintf(stderr, "      -T: number of reader threads (one input file each)\n");
  exit(1);
}

/* the first input without its directory-independent suffix: reads.fq -> reads */
static char *default_root(const char *name)
{ static const char *suffix[] = { ".fastq", ".fasta", ".fq", ".fa", ".fna", ".fas", NULL };
  int i;
  for (i = 0; suffix[i] != NULL; i++)
    { int epos = (int) strlen(name) - (int) strlen(suffix[i]);
      if (epos > 0 && strcasecmp(name + epos, suffix[i]) == 0) return strndup(name, (size_t) epos);
    }
  return strdup(name);
}

int main(int argc, char *argv[])
{ int verbose = 0, nthreads = 4, kmer = 31, minval = 4, do_hist = 0, nparts = 0;
  char *out = NULL, *root, *hname = NULL;
  int i, j;
  smg_count_opts opts;
  smg_count_stats st;
  smg_count_parts parts;
  uint64_t *keys = NULL, *hist;
  uint16_t *cnt = NULL;
  int64_t n = 0;
  int W = 0;
  char errbuf[1024];

  Prog_Name = "smg_count";
  j = 1;
  for (i = 1; i < argc; i++)
    if (argv[i][0] == '-' && argv[i][1] != '\0')
      switch (argv[i][1])
      { case 'v': verbose = 1; break;
        case 'H': do_hist = 1; break;
        case 'k': kmer = arg_positive(argv[i], "K-mer length"); break;
        case 'p':
          { char *eptr;
            long v = strtol(argv[i] + 2, &eptr, 10);
            if (argv[i][2] == '\0' || *eptr != '\0')
              { fprintf(stderr, "%s: -p '%s' argument is not an integer\n", Prog_Name, argv[i] + 2); exit(1); }
            if (v < 0 || v > SMG_COUNT_BINS)
              { fprintf(stderr, "%s: Number of key ranges must be 0 .. %d (%s)\n", Prog_Name, SMG_COUNT_BINS, argv[i] + 2); exit(1); }
            nparts = (int) v;
            break;
          }
        case 't': minval = arg_positive(argv[i], "Count threshold"); break;
        case 'T': nthreads = arg_positive(argv[i], "Number of threads"); if (nthreads > 16) nthreads = 16; break;
        case 'o': free(out); out = strdup(argv[i] + 2); if (out == NULL || out[0] == '\0') usage(); break;
        default:
          fprintf(stderr, "%s: -%c is an illegal option\n", Prog_Name, argv[i][1]);
          exit(1);
      }
    else
      argv[j++] = argv[i];
  if (j < 2) usage();
  if (kmer < SMG_COUNT_MIN_KMER || kmer > SMG_MAX_KMER)
    { fprintf(stderr, "%s: K-mer length must be %d .. %d (%d): the table has a 3-byte prefix index and keys of at most 4 words\n",
              Prog_Name, SMG_COUNT_MIN_KMER, SMG_MAX_KMER, kmer);
      exit(1);
    }
  if (minval > SMG_COUNT_MAX_COUNT)
    { fprintf(stderr, "%s: Count threshold must be at most %d (%d)\n", Prog_Name, SMG_COUNT_MAX_COUNT, minval); exit(1); }
  for (i = 1; i < j; i++)
    { FILE *f = fopen(argv[i], "rb");
      if (f == NULL) { fprintf(stderr, "%s: Cannot open %s for reading\n", Prog_Name, argv[i]); exit(1); }
      fclose(f);
    }
  root = out != NULL ? path_n_root(out, ".ktab") : default_root(argv[1]);
  hist = (uint64_t *) calloc(SMG_COUNT_HIST, sizeof(uint64_t));
  if (root == NULL || hist == NULL) { fprintf(stderr, "%s: Out of memory\n", Prog_Name); exit(1); }

  memset(&opts, 0, sizeof(opts));
  { const char *g = getenv("SMUDGEPLOT_GPU"); opts.device = g ? atoi(g) : 0; }
  opts.kmer = kmer; opts.minval = minval; opts.host_threads = nthreads; opts.verbose = verbose;
  memset(&parts, 0, sizeof(parts));
  parts.partitions = nparts;
  errbuf[0] = 0;
  if (smg_count_files_parts((const char *const *) (argv + 1), j - 1, &opts, &parts, &keys, &cnt, &n, &W, hist, &st, errbuf, sizeof(errbuf)) != SMG_OK)
    { fprintf(stderr, "%s: %s\n", Prog_Name, errbuf[0] ? errbuf : "GPU engine failed"); exit(1); }

  if (smg_cli_write_ktab(root, kmer, 3, 1, minval, keys, cnt, n, W))
    { smg_cli_remove_ktab(root, 1); exit(1); }
  if (do_hist)
    { int64_t c, top = 0;
      FILE *f;
      hname = (char *) malloc(strlen(root) + 16);
      if (hname == NULL) { smg_cli_remove_ktab(root, 1); fprintf(stderr, "%s: Out of memory\n", Prog_Name); exit(1); }
      sprintf(hname, "%s.hist.txt", root);
      for (c = 1; c < SMG_COUNT_HIST; c++) if (hist[c]) top = c;
      f = fopen(hname, "w");
      for (c = 1; f != NULL && c <= top; c++)
        if (fprintf(f, "%lld\t%llu\n", (long long) c, (unsigned long long) hist[c]) < 0) { fclose(f); f = NULL; }
      if (f == NULL || fclose(f))
        { fprintf(stderr, "%s: Cannot write %s\n", Prog_Name, hname);
          remove(hname); smg_cli_remove_ktab(root, 1);
          exit(1);
        }
    }
  if (verbose)
    { fprintf(stderr, "  %lld bases, %lld %d-mers, %lld distinct, %lld with count >= %d, %lld batch%s\n", (long long) st.bases,
              (long long) st.windows, kmer, (long long) st.distinct, (long long) st.kept, minval, (long long) st.batches,
              st.batches == 1 ? "" : "es");
      fprintf(stderr, "  %d key range%s, packed input %.3f GB on the device; ms: pack %.3f  plan %.3f\n", (int) parts.used,
              parts.used == 1 ? "" : "s", (double) parts.store_bytes * 1e-9, parts.ms_pack, parts.ms_plan);
      fprintf(stderr, "  ms: read %.1f  extract %.3f  sort %.3f  reduce+merge %.3f  finish %.3f  wall %.1f\n", st.ms_read, st.ms_extract,
              st.ms_sort, st.ms_reduce, st.ms_finish, st.ms_wall);
    }
  smg_count_free(keys); smg_count_free(cnt);
  free(hist); free(root); free(out); free(hname);
  exit(0);
}
