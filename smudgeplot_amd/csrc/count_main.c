/*******************************************************************************************
 *
 *  smg_count -- count the canonical k-mers of FASTA / FASTQ reads on the GPU and write them as a FastK
 *               k-mer table (format F: stub + one hidden part file, 3-byte prefix index), plus the
 *               k-mer count histogram that `smudgeplot cutoff` reads.  The reads are plain or block-gzipped (BGZF, what
 *               bgzip writes: inflated on the device), or unaligned BAM (PacBio HiFi reads: the bases of its primary
 *               records, unpacked on the device); any other gzip file is refused unless -g is given: that refusal is a
 *               tested contract of this program, so plain gzip (what gzip, pigz and a sequencer write) is read on request
 *               only, inflated on the device in parallel; -g changes nothing for plain, BGZF and BAM inputs of the same call.
 *
 *  The step in front of `hetmers`: where a smudgeplot run starts from reads, this stands in for FastK.  With -e it is
 *  that step and `hetmers` in one process: the counted table stays in device memory and is trimmed, closed under reverse
 *  complement and scanned for het-mer pairs there (smg_hetmers_run_device: in core, or in prefix shards of the closed table one
 *  after the other where it is too large for that), and <output>.smu is written as `hetmers -e` writes it from the table on disk.
 *
 *  With -d the inputs are k-mers that another tool has counted already: the text dumps of kmc_dump, `jellyfish dump -c` and
 *  `meryl print`, one line <k-mer><space or tab><count> per k-mer, plain, BGZF or (with -g) plain gzip; every line adds its count
 *  to the smaller of its k-mer and its reverse complement.  An option for the reason -g is one: a file that begins ACGT is
 *  refused without it, and that is tested.  -t, -H, -o, -n and -e mean what they mean for reads; -p must be 0 or 1.
 *
 *  An input may be a stream: the argument - is standard input, and an argument that is not a regular file (a FIFO, /dev/stdin,
 *  the /dev/fd/N of a shell's <(...)) is opened once and read forward only, told by its first bytes as a file is.  That is the way
 *  in for CRAM (samtools fastq x.cram | smg_count -oSample -), zstd, bzip2, xz and fasterq-dump --stdout.  Plain gzip on a stream
 *  is refused with or without -g.  A stream has no root name: -o is needed where the first input is one.
 *
 *  Usage: smg_count [-v] [-g] [-d] [-T<int(4)>] [-k<int(31)>] [-t<int(4)>] [-p<int(0)>] [-H] [-e<int>] [-n] [-o<output>] <reads> ...
 *           -k: k-mer length, 13 .. 128          -t: keep the k-mers with count >= t
 *           -H: also write <output>.hist.txt     -T: reader threads (one input file each, at most 16)
 *           -o: root name of the table; default is the root of the first input
 *           -p: key ranges to count in: 0 as many as the data need, 1 one pass, 2 .. 4096 that many
 *           -e: also write <output>.smu, the het-mer pairs of the k-mers with count >= e (e >= t); one device
 *           -n: write no table (with -e or -H only)
 *           -g: read plain gzip inputs too (SMG_COUNT_GZIP_SPAN, test hook: the compressed bytes of a span)
 *           -d: the inputs are k-mer dumps (k-mer, separator, count per line), not reads
 *
 *  SMUDGEPLOT_GPU picks the device; SMG_COUNT_MAX_ENTRIES (test hook) is max_entries of smg_count_parts.  No CPU fallback.
 *  A failed run leaves no table, histogram or .smu file behind.
 *
 ********************************************************************************************/

#include <sys/stat.h>
#include <unistd.h>

#include "smg_cli.h"
#include "smg_count.h"

static void usage(void)
{ fprintf(stderr, "\nUsage: %s [-v] [-g] [-d] [-T<int(4)>] [-k<int(31)>] [-t<int(4)>] [-p<int(0)>] [-H] [-e<int>] [-n] [-o<output>] <reads> ...\n", Prog_Name);
  fprintf(stderr, "\n");
  fprintf(stderr, "      -k: k-mer length (13 .. %d)\n", SMG_MAX_KMER);
  fprintf(stderr, "      -t: keep the k-mers that occur at least t times\n");
  fprintf(stderr, "      -p: count in this many ranges of canonical k-mers (0 .. %d): 0 as many as the data need, 1 one pass\n", SMG_COUNT_BINS);
  fprintf(stderr, "      -H: write the k-mer count histogram to <output>.hist.txt\n");
  fprintf(stderr, "      -e: write the het-mer pairs of the k-mers that occur at least e times to <output>.smu (e >= t),\n");
  fprintf(stderr, "            from the table in device memory: what hetmers -e writes from the table file\n");
  fprintf(stderr, "      -n: write no table (with -e or -H)\n");
  fprintf(stderr, "      -g: read plain gzip <reads> too (reads.fastq.gz as gzip or pigz write it), inflated on the device;\n");
  fprintf(stderr, "            without it such a file is refused, as always; plain, BGZF and BAM inputs are read the same either way\n");
  fprintf(stderr, "      -d: the inputs are k-mer dumps, not reads: text lines <k-mer><space or tab><count> as kmc_dump, jellyfish dump -c\n");
  fprintf(stderr, "            and meryl print write them (plain, BGZF, with -g plain gzip); -k must be their k, -p 0 or 1\n");
  fprintf(stderr, "      -o: root name for the output table\n");
  fprintf(stderr, "            default is root of the first <reads> argument\n");
  fprintf(stderr, "      -v: verbose mode\n");
  fprintf(stderr, "      -T: number of reader threads (one input file each)\n");
  fprintf(stderr, "\n");
  fprintf(stderr, "      <reads>: FASTA or FASTQ, plain or block-gzipped (BGZF), or unaligned BAM (the bases of its primary records);\n");
  fprintf(stderr, "            - is standard input, and a FIFO, /dev/stdin or <(...) is read as the stream it is, once and forward only:\n");
  fprintf(stderr, "            samtools fastq x.cram | %s -oSample -   (-o is needed where the first input is a stream; no plain gzip)\n", Prog_Name);
  exit(1);
}

/* the first input without its directory-independent suffix: reads.fq -> reads, reads.fq.gz -> reads, reads.bam -> reads */
static char *default_root(const char *name)
{ static const char *suffix[] = { ".fastq", ".fasta", ".fq", ".fa", ".fna", ".fas", ".bam", NULL };
  static const char *packed[] = { ".gz", ".bgz", NULL };
  int i, len = (int) strlen(name);
  for (i = 0; packed[i] != NULL; i++)
    { int epos = len - (int) strlen(packed[i]);
      if (epos > 0 && strcasecmp(name + epos, packed[i]) == 0) { len = epos; break; }
    }
  for (i = 0; suffix[i] != NULL; i++)
    { int epos = len - (int) strlen(suffix[i]);
      if (epos > 0 && strncasecmp(name + epos, suffix[i], strlen(suffix[i])) == 0) return strndup(name, (size_t) epos);
    }
  return strndup(name, (size_t) len);
}

/* standard input, or whatever stat does not call a regular file: a FIFO, /dev/stdin, the /dev/fd/N of a process substitution */
static int is_stream_arg(const char *name)
{ struct stat sb;
  return strcmp(name, "-") == 0 || (stat(name, &sb) == 0 && !S_ISREG(sb.st_mode));
}

/* remove what a run that fails half way has written */
static void remove_outputs(const char *root, int table, const char *hname, const char *sname)
{ if (table) smg_cli_remove_ktab(root, 1);
  if (hname != NULL) remove(hname);
  if (sname != NULL) remove(sname);
}

int main(int argc, char *argv[])
{ int verbose = 0, nthreads = 4, kmer = 31, minval = 4, do_hist = 0, nparts = 0, ethresh = 0, no_table = 0, gzip = 0, dump = 0;
  char *out = NULL, *root, *hname = NULL, *sname = NULL;
  int64_t *plot = NULL;
  smg_stats hst;
  int i, j;
  smg_count_opts opts;
  smg_count_stats st;
  smg_count_parts parts;
  uint64_t *keys = NULL, *hist;
  uint16_t *cnt = NULL;
  int64_t n = 0;
  int W = 0, shards = 1;
  char errbuf[1024];

  Prog_Name = "smg_count";
  j = 1;
  for (i = 1; i < argc; i++)
    if (argv[i][0] == '-' && argv[i][1] != '\0')
      switch (argv[i][1])
      { case 'v': verbose = 1; break;
        case 'H': do_hist = 1; break;
        case 'n': no_table = 1; break;
        case 'g': gzip = 1; break;
        case 'd': dump = 1; break;
        case 'e': ethresh = arg_positive(argv[i], "Error-mer threshold"); break;
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
  if (no_table && !do_hist && ethresh == 0)
    { fprintf(stderr, "%s: -n leaves nothing to write: give -e or -H with it\n", Prog_Name); usage(); }
  if (ethresh > 0 && ethresh < minval)
    { fprintf(stderr, "%s: -e%d is below -t%d: the k-mers that occur less than %d times are not counted into the table\n", Prog_Name,
              ethresh, minval, minval);
      exit(1);
    }
  /* a regular file is opened and closed once, as always; a stream is not (that would end the writer of a FIFO): stat and access */
  for (i = 1; i < j; i++)
    if (strcmp(argv[i], "-") != 0)
      { struct stat sb;
        if (stat(argv[i], &sb) != 0) { fprintf(stderr, "%s: Cannot open %s for reading\n", Prog_Name, argv[i]); exit(1); }
        if (S_ISREG(sb.st_mode))
          { FILE *f = fopen(argv[i], "rb");
            if (f == NULL) { fprintf(stderr, "%s: Cannot open %s for reading\n", Prog_Name, argv[i]); exit(1); }
            fclose(f);
          }
        else if (access(argv[i], R_OK) != 0) { fprintf(stderr, "%s: Cannot open %s for reading\n", Prog_Name, argv[i]); exit(1); }
      }
  if (out == NULL && is_stream_arg(argv[1]))
    { fprintf(stderr, "%s: -o is needed where the first input is a stream (%s)\n", Prog_Name, argv[1]); exit(1); }
  root = out != NULL ? path_n_root(out, ".ktab") : default_root(argv[1]);
  hist = (uint64_t *) calloc(SMG_COUNT_HIST, sizeof(uint64_t));
  if (root == NULL || hist == NULL) { fprintf(stderr, "%s: Out of memory\n", Prog_Name); exit(1); }

  memset(&opts, 0, sizeof(opts));
  { const char *g = getenv("SMUDGEPLOT_GPU"); opts.device = g ? atoi(g) : 0; }
  opts.kmer = kmer; opts.minval = minval; opts.host_threads = nthreads; opts.verbose = verbose; opts.gzip = gzip; opts.dump = dump;
  memset(&parts, 0, sizeof(parts));
  parts.partitions = nparts;
  { const char *m = getenv("SMG_COUNT_MAX_ENTRIES"); if (m != NULL && atoll(m) > 0) parts.max_entries = atoll(m); }   /* (test hook) */
  errbuf[0] = 0;
  memset(&hst, 0, sizeof(hst));
  if (ethresh == 0)
    { if (smg_count_files_parts((const char *const *) (argv + 1), j - 1, &opts, &parts, &keys, &cnt, &n, &W, hist, &st, errbuf, sizeof(errbuf)) != SMG_OK)
        { fprintf(stderr, "%s: %s\n", Prog_Name, errbuf[0] ? errbuf : "GPU engine failed");
          if (verbose) fprintf(stderr, "  nothing was written under the root name %s\n", root);
          exit(1);
        }
    }
  else
    { /* the table stays where it was counted; everything is computed before the first file is written */
      uint64_t *d_keys = NULL;
      uint16_t *d_cnt = NULL;
      smg_opts ho;
      int rc;
      if (smg_count_files_device((const char *const *) (argv + 1), j - 1, &opts, &parts, &d_keys, &d_cnt, &n, &W, hist, &st, errbuf, sizeof(errbuf)) != SMG_OK)
        { fprintf(stderr, "%s: %s\n", Prog_Name, errbuf[0] ? errbuf : "GPU engine failed");
          if (verbose) fprintf(stderr, "  nothing was written under the root name %s\n", root);
          exit(1);
        }
      plot = (int64_t *) malloc(sizeof(int64_t) * SMG_PLOT_CELLS);
      rc = plot == NULL ? SMG_ENOMEM : SMG_OK;
      if (rc == SMG_OK && !no_table)                              /* a host copy for the table file, through an engine */
        { smg_engine *e = smg_engine_create(opts.device, NULL, errbuf, sizeof(errbuf));
          keys = (uint64_t *) malloc(sizeof(uint64_t) * (size_t) (n > 0 ? n : 1) * (size_t) W);
          cnt = (uint16_t *) malloc(sizeof(uint16_t) * (size_t) (n > 0 ? n : 1));
          if (e == NULL) rc = SMG_ENODEV;
          else if (keys == NULL || cnt == NULL) rc = SMG_ENOMEM;
          else if ((rc = smg_engine_bind(e, kmer, n, d_keys, d_cnt, errbuf, sizeof(errbuf))) == SMG_OK)
            rc = smg_engine_table_host(e, keys, cnt, n, errbuf, sizeof(errbuf));
          smg_engine_destroy(e);
        }
      if (rc == SMG_OK)
        { memset(&ho, 0, sizeof(ho));
          ho.device = opts.device; ho.symcheck = SMG_SYM_HASH; ho.verbose = verbose; ho.ethresh = ethresh;
          ho.condition = SMG_COND_SYMM | (ethresh > minval ? SMG_COND_TRIM : 0);      /* (nothing below t is left to trim) */
          rc = smg_hetmers_run_device(kmer, n, d_keys, d_cnt, &ho, plot, &hst, errbuf, sizeof(errbuf));
          if (rc == SMG_OK && verbose)                             /* (the plan that call made, asked once more for the report) */
            { int32_t mode[3];
              if (smg_hetmers_run_device_mode(kmer, n, &ho, 0.0, mode, NULL, 0) == SMG_OK && mode[0] == SMG_MODE_SEQUENTIAL) shards = mode[1];
            }
        }
      smg_count_device_free(d_keys); smg_count_device_free(d_cnt);
      if (rc != SMG_OK)
        { fprintf(stderr, "%s: %s\n", Prog_Name, errbuf[0] ? errbuf : rc == SMG_ENOMEM ? "Out of memory" : "GPU engine failed");
          exit(1);
        }
    }

  if (!no_table && smg_cli_write_ktab(root, kmer, 3, 1, minval, keys, cnt, n, W))
    { smg_cli_remove_ktab(root, 1); exit(1); }
  if (do_hist)
    { int64_t c, top = 0;
      FILE *f;
      hname = (char *) malloc(strlen(root) + 16);
      if (hname == NULL) { remove_outputs(root, !no_table, NULL, NULL); fprintf(stderr, "%s: Out of memory\n", Prog_Name); exit(1); }
      sprintf(hname, "%s.hist.txt", root);
      for (c = 1; c < SMG_COUNT_HIST; c++) if (hist[c]) top = c;
      f = fopen(hname, "w");
      for (c = 1; f != NULL && c <= top; c++)
        if (fprintf(f, "%lld\t%llu\n", (long long) c, (unsigned long long) hist[c]) < 0) { fclose(f); f = NULL; }
      if (f == NULL || fclose(f))
        { fprintf(stderr, "%s: Cannot write %s\n", Prog_Name, hname);
          remove_outputs(root, !no_table, hname, NULL);
          exit(1);
        }
    }
  if (ethresh > 0)
    { sname = (char *) malloc(strlen(root) + 16);
      if (sname != NULL) sprintf(sname, "%s.smu", root);
      if (sname == NULL || smg_cli_write_smu(sname, plot, NULL))
        { fprintf(stderr, "%s: Cannot write %s.smu\n", Prog_Name, root);
          remove_outputs(root, !no_table, hname, sname);
          exit(1);
        }
    }
  if (verbose)
    { for (i = 1; i < j; i++)
        { int64_t blocks = 0, text = 0, spans = 0, linked = 0, repaired = 0;
          if (smg_count_gzip_report(argv[i], &blocks, &text, &spans, &linked, &repaired, NULL) == SMG_OK)
            fprintf(stderr, "  %s: gzip, %lld members, %lld text bytes, %lld of %lld spans linked, %lld repaired, inflated on the device\n", argv[i],
                    (long long) blocks, (long long) text, (long long) linked, (long long) spans, (long long) repaired);
          if (smg_count_bgzf_scan(argv[i], &blocks, &text, NULL, 0) == SMG_OK)
            fprintf(stderr, "  %s: BGZF, %lld blocks, %lld text bytes, inflated on the device\n", argv[i], (long long) blocks, (long long) text);
          if (smg_count_bam_report(argv[i], &blocks, &text, NULL) == SMG_OK)
            fprintf(stderr, "  %s: BAM, %lld records, %lld bases, unpacked on the device\n", argv[i], (long long) blocks, (long long) text);
        }
      if (dump) fprintf(stderr, "  k-mer dumps: %lld lines, decoded on the device\n", (long long) st.windows);
      fprintf(stderr, "  %lld bases, %lld %d-mers, %lld distinct, %lld with count >= %d, %lld batch%s\n", (long long) st.bases,
              (long long) st.windows, kmer, (long long) st.distinct, (long long) st.kept, minval, (long long) st.batches,
              st.batches == 1 ? "" : "es");
      fprintf(stderr, "  %d key range%s, packed input %.3f GB on the device; ms: pack %.3f  plan %.3f", (int) parts.used,
              parts.used == 1 ? "" : "s", (double) parts.store_bytes * 1e-9, parts.ms_pack, parts.ms_plan);
      if (parts.split > 0)
        fprintf(stderr, "; %d bin%s of six leading bases split on the next six", (int) parts.split, parts.split == 1 ? "" : "s");
      fprintf(stderr, "\n");
      fprintf(stderr, "  ms: read %.1f  extract %.3f  sort %.3f  reduce+merge %.3f  finish %.3f  wall %.1f\n", st.ms_read, st.ms_extract,
              st.ms_sort, st.ms_reduce, st.ms_finish, st.ms_wall);
      if (ethresh > 0)
        { fprintf(stderr, "  het-mers at -e%d: %lld entries in the closed table, %lld pairs; ms: conditioning %.3f  pairs %.3f", ethresh,
                  (long long) hst.nels, (long long) hst.npairs, hst.ms_decode, hst.ms_total);
          if (shards > 1) fprintf(stderr, "; %d prefix shards one after the other", shards);
          fprintf(stderr, "\n");
        }
    }
  if (ethresh == 0) { smg_count_free(keys); smg_count_free(cnt); }
  else { free(keys); free(cnt); }
  free(plot); free(sname);
  free(hist); free(root); free(out); free(hname);
  exit(0);
}
