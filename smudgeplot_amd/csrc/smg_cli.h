/* smg_cli.h -- what the two drop-in executables share: the argv conventions of Myers' ARG_* macros
 * (gene_core.h:32-55), path helpers, table loading with the reference's error messages, the conditioning
 * decision (examine_table + Logex/Symmex plan, PloidyPlot.c:1341-1426 == PloidyList.c:1351-1444) and the
 * engine options.  Header-only (static functions): each executable is one C file plus smg_ktab.c.
 */
#ifndef SMG_CLI_H
#define SMG_CLI_H

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <stdint.h>

#include "smg_hetmers.h"
#include "smg_ktab.h"

static const char *Prog_Name;          /* set by each main (ARG_INIT, gene_core.h:32-35) */

/* ARG_POSITIVE, gene_core.h:45-55 */
static int arg_positive(const char *arg, const char *name)
{ char *eptr;
  long  v = strtol(arg + 2, &eptr, 10);
  if (*eptr != '\0' || arg[2] == '\0')
    { fprintf(stderr, "%s: -%c '%s' argument is not an integer\n", Prog_Name, arg[1], arg + 2);
      exit(1);
    }
  if ((int) v <= 0)
    { fprintf(stderr, "%s: %s must be positive (%d)\n", Prog_Name, name, (int) v);
      exit(1);
    }
  return (int) v;
}

/* PathnRoot(name,".ktab"), gene_core.c */
static char *path_n_root(const char *name, const char *suffix)
{ int epos = (int) strlen(name) - (int) strlen(suffix);
  if (epos > 0 && strcasecmp(name + epos, suffix) == 0)
    return strndup(name, (size_t) epos);
  return strdup(name);
}

__attribute__((unused)) static void system_x(const char *command)       /* SystemX, gene_core.c:19-24 */
{ if (system(command) != 0)
    { fprintf(stderr, "%s: Command '%s' failed\n", Prog_Name, command);
      exit(1);
    }
}

static int Load_Threads = 1;           /* -T: host threads that read the part files */
static int Load_Lazy = 0;              /* 1: leave the records on disk (smg_ktab_open), the engine pulls them */

__attribute__((unused)) static void load_or_die(const char *name, smg_ktab *T)
{ char what[4096];
  switch (Load_Lazy ? smg_ktab_open(name, T, what) : smg_ktab_load_mt(name, T, what, Load_Threads))
  { case SMG_KTAB_OK:
      return;
    case SMG_KTAB_NOSTUB:
      fprintf(stderr, "%s: Cannot open k-mer table %s\n", Prog_Name, name);
      break;
    case SMG_KTAB_NOPART:
      fprintf(stderr, "%s: Table part %s is missing ?\n", Prog_Name, what);
      break;
    case SMG_KTAB_KMISMATCH:
      fprintf(stderr, "%s: Table part %s does not have k-mer length matching stub ?\n", Prog_Name, what);
      break;
    case SMG_KTAB_NOMEM:
      fprintf(stderr, "%s: Out of memory (Allocating k-mer table)\n", Prog_Name);
      break;
    default:
      fprintf(stderr, "%s: Table file %s is truncated or not a FastK table\n", Prog_Name, what);
      break;
  }
  exit(1);
}


/* parsed command line common to hetmers / extract_kmer_pairs */
typedef struct smg_cli
{ int   verbose, nthreads, ethresh;
  const char *sort_path;
  char *out;                   /* -o, or NULL */
  int   argc;                  /* positional arguments left in argv[1..argc-1] */
} smg_cli;

__attribute__((unused)) static void smg_cli_parse(int argc, char *argv[], smg_cli *c)
{ int flags[128];
  int i, j, k;
  c->nthreads = 4; c->ethresh = 4; c->sort_path = "/tmp"; c->out = NULL;
  for (i = 0; i < 128; i++) flags[i] = 0;
  j = 1;
  for (i = 1; i < argc; i++)
    if (argv[i][0] == '-')
      switch (argv[i][1])
      { default:                                   /* ARG_FLAGS("vklfs"), gene_core.h:37-43 */
          for (k = 1; argv[i][k] != '\0'; k++)
            { if (strchr("vklfs", argv[i][k]) == NULL)
                { fprintf(stderr, "%s: -%c is an illegal option\n", Prog_Name, argv[i][k]);
                  exit(1);
                }
              flags[(int) argv[i][k]] = 1;
            }
          break;
        case 'e':
          c->ethresh = arg_positive(argv[i], "Error-mer threshold");
          break;
        case 'o':
          free(c->out);
          c->out = strdup(argv[i] + 2);
          if (c->out == NULL) exit(1);
          break;
        case 'P':
          c->sort_path = argv[i] + 2;
          break;
        case 'T':
          c->nthreads = arg_positive(argv[i], "Number of threads");
          if (c->nthreads > 64)
            { fprintf(stderr, "%s: Warning, only 64 threads will be used\n", Prog_Name);
              c->nthreads = 64;
            }
          break;
      }
    else
      argv[j++] = argv[i];
  c->argc = j;
  c->verbose = flags['v'];
}

__attribute__((unused)) static void smg_cli_usage_tail(void)
{ fprintf(stderr, "\n");
  fprintf(stderr, "      -o: root name for output table\n");
  fprintf(stderr, "            default is root of <source> argument\n");
  fprintf(stderr, "\n");
  fprintf(stderr, "      -e: count threshold below which k-mers are considered erroneous\n");
  fprintf(stderr, "      -v: verbose mode\n");
  fprintf(stderr, "      -T: number of threads to use\n");
  fprintf(stderr, "      -P: Place all temporary files in directory -P.\n");
  exit(1);
}

/* Open the table, probe it, condition it (on the device by default, with FastK's tools when
   SMUDGEPLOT_USE_FASTK_TOOLS=1), fill the engine options.  Returns the name of a temporary
   conditioned table to Fastrm afterwards (malloc'ed) or NULL.   PloidyPlot.c:1341-1426          */
__attribute__((unused)) static char *smg_cli_open_table(const smg_cli *c, const char *SRC, smg_ktab *T, smg_opts *opts)
{ const char *troot = "";        /* mktemp("._SPAIR.XXXX") yields "" with 4 X's: temps are
                                    literally ".trim"/".symx" in the cwd  */
  int   trim, symm, use_tools = 0, condition = 0;
  char *tname   = (char *) malloc(strlen(SRC) + strlen(troot) + 10);
  char *command = (char *) malloc(strlen(SRC) + strlen(troot) + strlen(c->sort_path) + 100);
  char *input = NULL;

  if (tname == NULL || command == NULL)
    { fprintf(stderr, "%s: Out of memory (Allocating strings)\n", Prog_Name); exit(1); }

  Load_Threads = c->nthreads;
  load_or_die(SRC, T);
  switch (smg_ktab_examine_mt(T, c->ethresh, c->nthreads < 1 ? 1 : c->nthreads > 16 ? 16 : c->nthreads, &trim, &symm)   /* -T is honoured (1..16 probe threads) */)
  { case SMG_KTAB_OK:
      break;
    case SMG_KTAB_NOMEM:
      fprintf(stderr, "%s: Out of memory (Allocating k-mer table)\n", Prog_Name);
      exit(1);
    default:
      fprintf(stderr, "%s: Table file %s is truncated or not a FastK table\n", Prog_Name, SRC);
      exit(1);
  }

  if (c->verbose)
    { fprintf(stderr, "\n  The input table is");
      if (trim)
        fprintf(stderr, symm ? " trimmed and symmetric\n" : " trimmed but not symmetric\n");
      else
        fprintf(stderr, symm ? " untrimmed yet symmetric\n" : " untrimmed and not symmetric\n");
    }

  sprintf(tname, "%s", SRC);

  /* Conditioning.  The reference delegates it to FastK's Logex / Symmex / Fastrm through system(3)
     (PloidyPlot.c:1381-1414); those tools are not part of smudgeplot.  Here the same two steps run on
     the device right after the table is decoded (smg_opts.condition), with the same progress lines
     and no temporary tables.  SMUDGEPLOT_USE_FASTK_TOOLS=1 restores the reference's shell-outs
     (identical command strings, temp tables ".trim" / ".symx" in the cwd).                      */
  { const char *ft = getenv("SMUDGEPLOT_USE_FASTK_TOOLS");
    use_tools = ft != NULL && atoi(ft) != 0;
  }
  if (!trim)
    { if (c->verbose)
        { fprintf(stderr, "\n  Trimming k-mers in table with count < %d\n", c->ethresh); fflush(stderr); }
      if (use_tools)
        { sprintf(command, "Logex -T%d '%s.trim=A[%d-]' %s", c->nthreads, troot, c->ethresh, tname);
          system_x(command);
          sprintf(tname, "%s.trim", troot);
        }
      else condition |= SMG_COND_TRIM;
    }
  if (!symm)
    { if (c->verbose)
        { fprintf(stderr, trim ? "\n  Making table symmetric\n" : "\n  Making trimmed table symmetric\n");
          fflush(stderr);
        }
      if (use_tools)
        { sprintf(command, "Symmex -T%d -P%s %s %s.symx", c->nthreads, c->sort_path, tname, troot);
          system_x(command);
          if (!trim)
            { sprintf(command, "Fastrm %s.trim", troot);
              system_x(command);
            }
          sprintf(tname, "%s.symx", troot);
        }
      else condition |= SMG_COND_SYMM;
    }
  if (use_tools && !(symm && trim))
    { input = strdup(tname);
      smg_ktab_free(T);
      load_or_die(input, T);
    }
  free(command);
  free(tname);

  memset(opts, 0, sizeof(*opts));
  { const char *g = getenv("SMUDGEPLOT_GPU"), *s = getenv("SMUDGEPLOT_SYMCHECK"), *ng = getenv("SMUDGEPLOT_GPUS");
    opts->device = g ? atoi(g) : 0;
    opts->ngpus = ng ? atoi(ng) : 0;          /* > 1: prefix-shard the table over that many GPUs of the node */
    opts->symcheck = SMG_SYM_HASH;
    if (s && strcasecmp(s, "exact") == 0) opts->symcheck = SMG_SYM_EXACT;
    if (s && strcasecmp(s, "none") == 0) opts->symcheck = SMG_SYM_NONE;
    opts->verbose = c->verbose;
    opts->condition = condition;
    opts->ethresh = c->ethresh;
  }
  return input;
}

/* the table as a source the engine pulls from (records still on disk, or already in memory) */
__attribute__((unused)) static int smg_cli_source_read(void *ctx, int part, int64_t first, int64_t nent, void *dst)
{ return smg_ktab_read((const smg_ktab *) ctx, part, first, nent, dst); }

__attribute__((unused)) static void smg_cli_table_source(const smg_ktab *T, smg_table_source *src, int nthreads)
{ const char *io = getenv("SMUDGEPLOT_IO_THREADS");
  src->kmer = T->kmer; src->ibyte = T->ibyte; src->nparts = T->nparts; src->minval = T->minval;
  src->nels = T->nels;
  src->part_nels = T->part_nels;
  src->prefix_index = T->index;
  src->read = smg_cli_source_read;
  src->ctx = (void *) T;
  /* readers: EIGHT, whatever -T says -- pulling the part files out of the page cache is all the host does for this
     engine; 4 threads (the CLI's default) leave the PCIe link two thirds idle, and more than 8 get in each other's
     way (32 readers: 22.7 instead of 40 GB/s, 0.77 instead of 0.52 s for the 1e9-entry table,
     profiles/r03_e2e_1e9_entries.json).  -T still sets the threads of the conditioning probe; SMUDGEPLOT_IO_THREADS
     overrides the readers.                                                                                      */
  (void) nthreads;
  src->host_threads = io != NULL && atoi(io) > 0 ? atoi(io) : 8;
  if (src->host_threads > 64) src->host_threads = 64;
}

__attribute__((unused)) static void smg_cli_table_view(const smg_ktab *T, smg_table_view *tv)
{ tv->kmer = T->kmer; tv->ibyte = T->ibyte; tv->nparts = T->nparts; tv->minval = T->minval;
  tv->nels = T->nels;
  tv->part_data = (const uint8_t *const *) T->part;
  tv->part_nels = T->part_nels;
  tv->prefix_index = T->index;
}

static int smg_cli_write_all(FILE *f, const void *p, size_t n) { return fwrite(p, 1, n, f) == n ? 0 : -1; }

/* Write a sorted, duplicate-free table as format F (libfastk.c:786-908 reads it back): stub = kmer, nparts, minval,
   ibyte, index[]; part p = kmer, n_p, n_p records of (hbyte suffix bytes + uint16 count).  keys: n entries of W
   left-aligned 64-bit words.  target: root name, with or without ".ktab".  0, or -1 after a message on stderr.   */
__attribute__((unused)) static int smg_cli_write_ktab(const char *target, int kmer, int ibyte, int nparts_in, int minval,
                                                      const uint64_t *keys, const uint16_t *cnt, int64_t n, int W)
{ const int kbyte = (kmer + 3) >> 2, hbyte = kbyte - ibyte, pbyte = hbyte + 2;
  const int nparts = nparts_in > 0 ? nparts_in : 1;
  const int64_t ixlen = (int64_t) 1 << (8 * ibyte);
  int64_t *index = (int64_t *) calloc((size_t) ixlen, sizeof(int64_t));
  int64_t *cut = (int64_t *) malloc(sizeof(int64_t) * (size_t) (nparts + 1));
  uint8_t *rec = (uint8_t *) malloc((size_t) (n > 0 ? n : 1) * pbyte);
  char *root = path_n_root(target, ".ktab");
  const char *slash = root ? strrchr(root, '/') : NULL;
  char *dir = root == NULL ? NULL : slash ? strndup(root, (size_t) (slash - root)) : strdup(".");
  const char *base = slash ? slash + 1 : root;
  char *path = root ? (char *) malloc(strlen(root) + 64) : NULL;
  int64_t e, p;
  int32_t hdr[4];
  int rc = 0;
  FILE *f;
  if (!index || !cut || !rec || !root || !dir || !path)
    { fprintf(stderr, "%s: Out of memory (Allocating k-mer table)\n", Prog_Name); rc = -1; }
  if (rc == 0)
    { for (e = 0; e < n; e++)
        { uint8_t kb[SMG_MAX_KMER / 4 + 8];
          int64_t pre = 0;
          int b;
          for (b = 0; b < kbyte; b++) kb[b] = (uint8_t) (keys[e * W + (b >> 3)] >> (56 - 8 * (b & 7)));
          for (b = 0; b < ibyte; b++) pre = (pre << 8) | kb[b];
          index[pre] += 1;
          memcpy(rec + (size_t) e * pbyte, kb + ibyte, (size_t) hbyte);
          rec[(size_t) e * pbyte + hbyte] = (uint8_t) (cnt[e] & 0xFF);
          rec[(size_t) e * pbyte + hbyte + 1] = (uint8_t) (cnt[e] >> 8);
        }
      for (p = 1; p < ixlen; p++) index[p] += index[p - 1];            /* cumulative END offsets */
      cut[0] = 0; cut[nparts] = n;
      for (p = 1; p < nparts; p++)                                      /* parts break on prefix boundaries */
        { const int64_t want = n / nparts * p;
          int64_t lo = 0, hi = ixlen - 1;
          while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (index[m] < want) lo = m + 1; else hi = m; }
          cut[p] = index[lo] > cut[p - 1] ? index[lo] : cut[p - 1];
        }
      sprintf(path, "%s/%s.ktab", dir, base);
      f = fopen(path, "wb");
      hdr[0] = kmer; hdr[1] = nparts; hdr[2] = minval; hdr[3] = ibyte;
      if (f == NULL || smg_cli_write_all(f, hdr, sizeof(hdr)) || smg_cli_write_all(f, index, sizeof(int64_t) * (size_t) ixlen) || fclose(f))
        { fprintf(stderr, "%s: Cannot write %s\n", Prog_Name, path); rc = -1; }
      for (p = 0; p < nparts && rc == 0; p++)
        { const int64_t np = cut[p + 1] - cut[p];
          const int32_t km = kmer;
          sprintf(path, "%s/.%s.ktab.%d", dir, base, (int) p + 1);
          f = fopen(path, "wb");
          if (f == NULL || smg_cli_write_all(f, &km, 4) || smg_cli_write_all(f, &np, 8)
              || smg_cli_write_all(f, rec + (size_t) cut[p] * pbyte, (size_t) np * pbyte) || fclose(f))
            { fprintf(stderr, "%s: Cannot write %s\n", Prog_Name, path); rc = -1; }
        }
    }
  free(index); free(cut); free(rec); free(root); free(dir); free(path);
  return rc;
}

/* remove the stub and the part files 1..nparts of a table (a run that failed half way leaves none behind) */
__attribute__((unused)) static void smg_cli_remove_ktab(const char *target, int nparts)
{ char *root = path_n_root(target, ".ktab");
  const char *slash = root ? strrchr(root, '/') : NULL;
  char *path = root ? (char *) malloc(2 * strlen(root) + 64) : NULL;
  int p;
  if (path != NULL)
    { sprintf(path, "%s.ktab", root);
      remove(path);
      for (p = 1; p <= nparts; p++)
        { if (slash) sprintf(path, "%.*s/.%s.ktab.%d", (int) (slash - root), root, slash + 1, p);
          else sprintf(path, ".%s.ktab.%d", root, p);
          remove(path);
        }
    }
  free(root); free(path);
}

/* The .smu writer, PloidyPlot.c:1603-1617: rows "min <tab> sum - min <tab> pairs" of the non-empty cells, sum ascending, min
   ascending, min == 500 never printed.  mark (may be NULL) is told 1 once the file is open and 2 once it is closed: a program
   that can be signalled over its output keeps track with it.  0; -1 when fname cannot be opened (the caller says so in its own
   words), -2 when a row or the close failed.                                                                          */
__attribute__((unused)) static int smg_cli_write_smu(const char *fname, const int64_t *plot, void (*mark)(int))
{ FILE *f = fopen(fname, "w");
  int a, i, bad = 0;
  if (f == NULL) return -1;
  if (mark != NULL) mark(1);
  for (a = 0; a <= SMG_SMAX; a++)
    for (i = 0; i < SMG_FMAX; i++)
      if (plot[a * SMG_PLOT_COLS + i] > 0)
        bad |= fprintf(f, "%i\t%i\t%lld\n", i, a - i, (long long) plot[a * SMG_PLOT_COLS + i]) < 0;
  bad |= fclose(f) != 0;
  if (mark != NULL) mark(2);
  return bad ? -2 : 0;
}

__attribute__((unused)) static void smg_cli_remove_temp(char *input)
{ if (input != NULL)
    { char *command = (char *) malloc(strlen(input) + 100);
      if (command == NULL) exit(1);
      sprintf(command, "Fastrm %s", input);
      system_x(command);
      free(command);
      free(input);
    }
}

#endif
