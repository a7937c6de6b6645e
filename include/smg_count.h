/* smg_count.h -- C ABI of the k-mer counter (libsmg_count.so, gfx950).
 *
 * Reads in, canonical k-mer table out: what FastK does in front of `hetmers`, on one MI355X.
 *   - input: FASTA / FASTQ (first byte '>' or '@'), plain or block-gzipped (BGZF, what bgzip and htslib write: a gzip
 *     file of independent members of at most 64 KiB, found by the BC subfield of its first header), every file of a call
 *     routed by its own header; the members of a BGZF file are inflated on the device and their CRC-32 checked there;
 *     any other gzip file is refused (SMG_EINVAL: recompress it with bgzip, or decompress it) -- unless the call opts in:
 *   - input: plain gzip (what gzip, pigz and a sequencer write: reads_1.fastq.gz), only where smg_count_opts.gzip is set.  The
 *     refusal above is a tested contract of this library and of smg_count (its message, and -z staying illegal), so reading
 *     such files is an option (smg_count -g) and not the default; it changes nothing for the plain, BGZF and BAM files of the
 *     same call.  A member is one DEFLATE stream; it is inflated in parallel all the same: the file is cut into spans, a
 *     wavefront finds a block start in each and decodes from there with the 32 KiB in front of it unknown, the spans are
 *     chained (what does not chain is decoded again from the known end in front of it), and a second pass decodes exactly
 *     between the restart points that the first one left, where the file is read (smg_gzip.hpp).  Every member's CRC-32 and
 *     ISIZE are checked; FEXTRA, FNAME, FCOMMENT, FHCRC, several members and trailing zero bytes are accepted.  One
 *     refusal (SMG_EINVAL, offset named): a single deflate block larger than one piece of the first pass (256 spans) or
 *     inflating to more than the text of one call (4 x SMG_COUNT_BGZF_CHUNK);
 *   - input: unaligned BAM (what PacBio HiFi reads are delivered in: a BGZF file whose text begins BAM\1), found by those
 *     four bytes; its records are framed on the host and their 4-bit sequences unpacked on the device.  Its stripped stream:
 *     in file order every record whose FLAG has neither 0x100 nor 0x800 set gives its l_seq bases, each code mapped through
 *     "=ACMGRSVTWYHKDBN", one SMG_COUNT_SEPARATOR between two such records -- the stream of a FASTA file of the same reads.
 *     The size of a BAM file bounds its bases as that of any BGZF file does, by the sum of its ISIZE fields: an over-estimate
 *     by 1.5 or more, so a large BAM may be counted by key range where one pass would have done; the result is the same
 *     whichever way it is counted.  CRAM is not gzip and, given as a file, is refused like any file that is neither FASTA nor
 *     FASTQ: it is read through a pipe (samtools fastq x.cram | smg_count ... -, or samtools view -u for BAM), see next;
 *   - input: streams.  A path that fstat does not call a regular file -- a FIFO, a socket, /dev/stdin, the /dev/fd/N of a shell's
 *     process substitution -- and the path "-" (standard input, at most once per call: a second one is SMG_EINVAL) is read
 *     once and forward only: opened once, told by its first bytes as a file is (plain FASTA / FASTQ, BGZF, BAM inside BGZF, with
 *     the dump option a dump), inflated and unpacked by the same kernels.  That is how CRAM, zstd, bzip2, xz and fasterq-dump
 *     reach the counter without a codec each.  Plain gzip on a stream is refused with or without smg_count_opts.gzip (its
 *     restart index reads the file twice: give the file, or decompress in the pipe).  A stream has no size, so a call with one
 *     has no bound: smg_count_stream_plan plans it, the packed store grows as the stream goes on, and the result is that of
 *     the same bytes read from a file.  A BGZF stream that ends inside a header or a member is SMG_EFORMAT, "<path>: BGZF
 *     block at offset <o>: the member (the header) is cut off by the end of the stream", o counted from its first byte.  The
 *     calls that read a file twice or seek in it (smg_count_bgzf_scan, smg_count_bgzf_inflate, smg_count_bam_strip,
 *     smg_count_gzip_inflate, smg_count_gzip_text_host) refuse a stream: SMG_EINVAL, "<path> is a stream: this call reads a file";
 *   - input: k-mers that another tool has counted already, only where smg_count_opts.dump is set (smg_count -d): the text
 *     that kmc_dump, `jellyfish dump -c` and `meryl print` write, one line per k-mer.  The refusal of a file that begins ACGT
 *     is a tested contract like that of plain gzip, hence the option; with it EVERY file of the call is a dump, its text routed
 *     by its own header as above (plain; BGZF; with gzip also set, plain gzip).  A file whose text begins with '>', '@', BAM\1
 *     or any byte outside ACGTacgt is SMG_EINVAL: the message names it and says that a call with the dump option reads dumps
 *     only.  The grammar of a line is strict: k bases ACGTacgt, exactly one ' ' or '\t', 1 .. 20 decimal digits, an optional
 *     '\r', '\n' (the last line may end with the text instead), at most SMG_COUNT_DUMP_LINE bytes.  The value saturates at
 *     2^32 - 1, leading zeros are fine, 0 is an error (hist[0] is 0).  The lines are decoded on the device.  Anything else is
 *     SMG_EFORMAT, "<path>: dump line at offset <o>: <reason>", o the offset of the first byte of the first bad line of that
 *     file in its (inflated) text, the reason one of
 *         is not <k> bases and a separator (is k right?)  |  has no count  |  count is 0  |  count is not followed by a line end
 *     Every line adds its count to the smaller of its k-mer and its reverse complement; the sums saturate (never wrap) and
 *     clamp at 32767 in the table.  A dump of both strands, repeated k-mers and several dumps in one call just add up.
 *     stats.windows is the number of lines, stats.bases k times that.  One pass only (the packed store is a store of reads):
 *     partitions must be 0 or 1, and where the sizes of the files (a line has k + 3 bytes at least) do not guarantee that one
 *     merge holds the lines -- 2^32 - 16 entries, or the memory a merge is priced at -- the call is refused with SMG_ENOMEM
 *     before its first allocation, the figures in the message.  SMG_COUNT_BATCH_BASES (test hook) is the batch in text bytes
 *     here, raised to SMG_COUNT_DUMP_LINE where it is smaller;
 *   - bases ACGTacgt code to 0..3, every other byte ends the current stretch, no k-mer spans two records;
 *   - every window of k bases counts once for the smaller of the k-mer and its reverse complement
 *     (left-aligned big-endian words, the order of the FastK table);
 *   - counts saturate at 32767; the table holds the k-mers with count >= t, sorted, one entry each;
 *   - hist[c] = number of distinct canonical k-mers with count c BEFORE trimming, c = 1..32767
 *     (the last bin holds the saturated ones, hist[0] is 0).
 * The result does not depend on the number of host threads, the batch size, the order of the files or the number of
 * key ranges the run is partitioned into, nor on where their ends lie.
 * Error codes are those of smg_hetmers.h.  No CPU fallback: without a HIP device the counting calls
 * return SMG_ENODEV; smg_count_parse and smg_count_dump_parse (plain files and plain streams only), smg_count_bgzf_scan, smg_count_bam_text,
 * smg_count_gzip_text_host, the plans and smg_count_version need no device.
 */
#ifndef SMG_COUNT_H
#define SMG_COUNT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef SMG_OK
#define SMG_OK        0
#define SMG_ENODEV   -1      /* no usable HIP device / HIP runtime error                     */
#define SMG_EINVAL   -2      /* bad argument (k out of range, unreadable or compressed file)  */
#define SMG_ENOMEM   -3      /* device or host allocation failed, distinct k-mers do not fit  */
#define SMG_EFORMAT  -4
#define SMG_ENOTSYM  -5
#endif
#ifndef SMG_MAX_KMER
#define SMG_MAX_KMER  128
#endif

#define SMG_COUNT_MIN_KMER   13        /* ibyte = 3: kbyte must exceed it              */
#define SMG_COUNT_MAX_COUNT  32767
#define SMG_COUNT_HIST       32768     /* hist[0 .. 32767]                              */
#define SMG_COUNT_SEPARATOR  '\n'      /* the byte between two records of a stripped stream */
#define SMG_COUNT_BIN_BITS   12        /* key ranges are cut between bins of the leading 12 bits  */
#define SMG_COUNT_BINS       4096      /* of the canonical k-mer                                  */
#define SMG_COUNT_FINE_BITS  24        /* a bin with more windows than one merge holds is split on its next 12 bits: */
#define SMG_COUNT_FINE_BINS  (1 << SMG_COUNT_FINE_BITS)   /* the ends of a range are values of the leading 24 bits  */
#define SMG_COUNT_BGZF_CHUNK (16 << 20)  /* compressed bytes of a BGZF file that one launch of the inflate kernel takes (whole
                                            members; a reader thread holds one such buffer and 4 x as much for their text) */
#define SMG_COUNT_BAM_TILE   4096      /* stripped bytes of a BAM file that one workgroup of the unpack kernel writes */
#define SMG_COUNT_DUMP_LINE  151       /* the longest legal line of a k-mer dump: 128 bases, a separator, 20 digits, \r\n */

typedef struct smg_count_opts
{ int32_t kmer;          /* 13 .. SMG_MAX_KMER                                   */
  int32_t minval;        /* t: keep the k-mers with count >= t (>= 1)            */
  int32_t device;        /* HIP device ordinal                                   */
  int32_t host_threads;  /* reader threads, one file each, at most 16 are used  */
  int32_t verbose;
  int32_t gzip;          /* 0: a gzip file that is not BGZF is refused, as always; 1: it is read (see the top of this file) */
  int32_t dump;          /* 0: the files are reads, as always; 1: every file is a k-mer dump (see the top of this file)      */
} smg_count_opts;

typedef struct smg_count_stats
{ int64_t bases;         /* sequence bytes read (separators not counted)         */
  int64_t windows;       /* k-mer instances counted                              */
  int64_t distinct;      /* distinct canonical k-mers                            */
  int64_t kept;          /* entries with count >= t                              */
  int64_t batches;
  double  ms_read;       /* start until the last reader delivered its last block (overlaps the device work) */
  double  ms_extract;    /* device events, summed over the batches               */
  double  ms_sort;
  double  ms_reduce;     /* runs of the batch + merge into the distinct list     */
  double  ms_finish;     /* histogram, clamp, trim                               */
  double  ms_wall;
} smg_count_stats;

/* Counting by key range.  Where one merge is not guaranteed to hold the distinct k-mers of the input, the input is
   read once, kept on the device at 3 bits per base, and counted one contiguous range of canonical k-mers at a time;
   the result is that of one pass.  partitions = 1 is today's single pass and refuses (SMG_ENOMEM) what does not fit.
   Ranges are cut between the bins of the leading 12 bits of the canonical k-mer.  In automatic mode a bin that alone holds
   more windows than one merge holds entries is split into the 4096 sub-bins of its next 12 bits, and a range may begin or
   end inside it; refused (SMG_ENOMEM, bin and sub-bin named) is only a single sub-bin above one merge: windows that share
   their twelve leading bases, a homopolymer run.  partitions = 2 .. SMG_COUNT_BINS cuts between whole bins only.        */
typedef struct smg_count_parts
{ int32_t partitions;    /* in: 0 automatic (one pass where the size of the input guarantees that it fits, else ranges
                                cut so that none can overflow a merge), 1 one pass, 2 .. SMG_COUNT_BINS that many ranges
                                of equal window share                                                               */
  int64_t max_entries;   /* in: test hook, plan and refuse as if one merge held only this many entries; 0: the device's
                                own limit                                                                           */
  int32_t used;          /* out: ranges the run was cut into (1: one pass, nothing was packed)                      */
  int64_t store_bytes;   /* out: device memory of the packed input                                                  */
  double  ms_pack;       /* out: device events, packing the batches into the store                                  */
  double  ms_plan;       /* out: host clock, window histograms over the store and the choice of the cuts           */
  int32_t split;         /* out: bins of the leading 12 bits that were split on their next 12 bits (0: every range is
                                whole bins); `used` counts all ranges                                                */
} smg_count_parts;

/* *keys: malloc'ed *nels * *key_words uint64, left aligned, sorted; *counts: malloc'ed uint16[*nels];
   hist: caller's uint64[SMG_COUNT_HIST] or NULL; stats may be NULL.  Release with smg_count_free.  */
int smg_count_files(const char *const *paths, int npaths, const smg_count_opts *opts,
                    uint64_t **keys, uint16_t **counts, int64_t *nels, int *key_words,
                    uint64_t *hist, smg_count_stats *stats, char *errbuf, size_t errlen);

/* the same from a host buffer of sequence bytes in which any byte outside ACGTacgt separates */
int smg_count_bases(const uint8_t *seq, int64_t n, const smg_count_opts *opts,
                    uint64_t **keys, uint16_t **counts, int64_t *nels, int *key_words,
                    uint64_t *hist, smg_count_stats *stats, char *errbuf, size_t errlen);

/* the same two with the partitioning under the caller's control; parts may be NULL (automatic).  stats->batches counts
   the sorted batches of all ranges and the stage times sum over the ranges.                                          */
int smg_count_files_parts(const char *const *paths, int npaths, const smg_count_opts *opts, smg_count_parts *parts,
                          uint64_t **keys, uint16_t **counts, int64_t *nels, int *key_words,
                          uint64_t *hist, smg_count_stats *stats, char *errbuf, size_t errlen);
int smg_count_bases_parts(const uint8_t *seq, int64_t n, const smg_count_opts *opts, smg_count_parts *parts,
                          uint64_t **keys, uint16_t **counts, int64_t *nels, int *key_words,
                          uint64_t *hist, smg_count_stats *stats, char *errbuf, size_t errlen);

/* the same two with the table left in DEVICE memory, for a consumer on the same device (smg_engine_bind,
   smg_hetmers_run_device of smg_hetmers.h): *d_keys = *nels * *key_words uint64 and *d_counts = uint16[*nels] are device
   pointers, each a whole hipMalloc allocation (never NULL on success, also for an empty table) -- release both with
   smg_count_device_free.  hist, stats and parts as above.  A partitioned run appends the kept entries of every range to the
   table on the device, which grows as the packed input does; a table that does not fit there next to the input is refused
   with SMG_ENOMEM, both sizes in the message, and never moved to the host behind the caller's back.                  */
int smg_count_files_device(const char *const *paths, int npaths, const smg_count_opts *opts, smg_count_parts *parts,
                           uint64_t **d_keys, uint16_t **d_counts, int64_t *nels, int *key_words,
                           uint64_t *hist, smg_count_stats *stats, char *errbuf, size_t errlen);
int smg_count_bases_device(const uint8_t *seq, int64_t n, const smg_count_opts *opts, smg_count_parts *parts,
                           uint64_t **d_keys, uint16_t **d_counts, int64_t *nels, int *key_words,
                           uint64_t *hist, smg_count_stats *stats, char *errbuf, size_t errlen);
void smg_count_device_free(void *d);

/* host only: the cuts of a partitioned run.  windows[SMG_COUNT_BINS] = windows per bin of the leading bits of the
   canonical k-mer.  partitions = 0: the fewest contiguous ranges none of which holds more than `budget` windows
   (greedy; a single bin above the budget is refused with SMG_ENOMEM and named in the message); 1: one range;
   2 .. SMG_COUNT_BINS: that many non-empty ranges of bins, as close to an equal share of the windows as the bins allow
   (budget is not looked at).  Range r is bins cuts[r] .. cuts[r + 1] - 1; cuts has room for SMG_COUNT_BINS + 1 values,
   cuts[0] = 0 and cuts[*nranges] = SMG_COUNT_BINS.                                                                  */
int smg_count_plan(const uint64_t *windows, int64_t budget, int32_t partitions, int32_t *cuts, int32_t *nranges,
                   char *errbuf, size_t errlen);

/* host only: the cuts where smg_count_plan refuses a single bin.  split[nsplit] = the bins that are split, ascending;
   sub[s * SMG_COUNT_BINS + j] = windows of bin split[s] whose next 12 bits are j (they add up to windows[split[s]]).
   The bins that are not split and the sub-bins of those that are form one ascending sequence of units; as in
   smg_count_plan a range takes units while its windows stay within `budget`, which gives the fewest contiguous ranges.
   Range r holds the canonical k-mers whose leading SMG_COUNT_FINE_BITS bits lie in cuts[r] .. cuts[r + 1] - 1;
   cuts[0] = 0, cuts[*nranges] = SMG_COUNT_FINE_BINS, and a cut that is no multiple of SMG_COUNT_BINS lies inside a split
   bin.  cuts has room for cuts_cap values: 2 * (sum of windows) / budget + 3 are enough, and SMG_COUNT_FINE_BINS + 1
   always are.  A sub-bin above the budget is refused with SMG_ENOMEM: the message is that of smg_count_plan for its bin,
   then the sub-bin, its twelve leading bases and its windows.  A bin above the budget that is not in `split` is
   SMG_EINVAL.                                                                                                        */
int smg_count_plan_fine(const uint64_t *windows, const int32_t *split, int32_t nsplit, const uint64_t *sub, int64_t budget,
                        int32_t *cuts, int64_t cuts_cap, int32_t *nranges, char *errbuf, size_t errlen);

/* host only: how a run shares out the device memory, before its first allocation -- the function the counting calls use
   themselves, with nothing read from the device or the environment.  kmer: k; free_bytes: free device memory; bound: the
   most sequence bytes the input can hold; partitions, max_entries: as in smg_count_parts; batch_bases: the value of the
   test hook SMG_COUNT_BATCH_BASES (bases per batch), 0 for none.  *cap = positions a batch holds; *parted = 0 for one
   pass, 1 where the batches are packed into a store and counted by key range; *store_cap = positions of that store (a
   multiple of 4096; 0 for one pass).  SMG_ENOMEM where the store, or the batch next to it, does not fit: the message
   names what is needed and what is free.                                                                             */
int smg_count_memory_plan(int32_t kmer, uint64_t free_bytes, int64_t bound, int32_t partitions, int64_t max_entries,
                          int64_t batch_bases, int64_t *cap, int32_t *parted, int64_t *store_cap, char *errbuf, size_t errlen);

/* host only: the plan of a call that reads at least one stream, which has no bound -- again the function the counting
   calls use themselves.  known_bound: the most sequence bytes the REGULAR files of the call can hold; store_bases: the value
   of the test hook SMG_COUNT_STREAM_STORE (positions the store begins with), 0 for none; the rest as above.
   partitions == 1: one pass, *parted = 0, *store_cap = 0, and *cap is the batch of smg_count_memory_plan without its clamp
   to the input; a distinct list that does not fit is refused by the merge that meets it (SMG_ENOMEM, its figures in the
   message), not in advance.  Any other value, 0 included: *parted = 1, the batches are packed and counted by key range.
   *store_cap = the positions the store BEGINS with, a multiple of 4096: store_bases rounded up, or without the hook 2^30
   (384 MiB), or what smg_count_memory_plan gives a store for known_bound where that is more.  The store then grows by half
   with a copy on the device; a growth that does not fit is SMG_ENOMEM, the message naming the positions packed so far, what
   the next size needs and what is free.  With no stream in the call smg_count_memory_plan decides, as it always did.       */
int smg_count_stream_plan(int32_t kmer, uint64_t free_bytes, int64_t known_bound, int32_t partitions, int64_t max_entries,
                          int64_t batch_bases, int64_t store_bases, int64_t *cap, int32_t *parted, int64_t *store_cap,
                          char *errbuf, size_t errlen);

/* host only: the stripped byte stream of one plain file or stream, the sequence of every record with line ends removed
   and one SMG_COUNT_SEPARATOR between two records.  *seq is malloc'ed (smg_count_free).  BGZF is
   SMG_EINVAL here (no device: see smg_count_bgzf_inflate).                                         */
int smg_count_parse(const char *path, uint8_t **seq, int64_t *n, char *errbuf, size_t errlen);

/* host only: the members of a BGZF file, walked from header to header.  SMG_OK: *blocks = members (empty ones and the EOF
   marker included), *text_bytes = the sum of their ISIZE fields.  SMG_EINVAL for a file that is not BGZF: the message of the
   counting calls for another gzip file, "<path> is not BGZF ..." for a file that is not gzip.  SMG_EFORMAT,
   "<path>: BGZF block at offset <o>: <reason>", for a header cut off by the end of the file, a BSIZE that reaches past it,
   an ISIZE above 65536 and a later member that is not BGZF.  The counting calls refuse the same before they touch the device. */
int smg_count_bgzf_scan(const char *path, int64_t *blocks, int64_t *text_bytes, char *errbuf, size_t errlen);

/* the text of a whole BGZF file, inflated by the kernel on `device` as the counting calls inflate it: *text is malloc'ed
   (smg_count_free), *n its bytes, *ms_kernel (may be NULL) the sum of the HIP-event times of the launches.  Errors as
   smg_count_bgzf_scan, and SMG_EFORMAT "<path>: BGZF block at offset <o>: <reason>" for the first member that does not
   inflate to ISIZE bytes with the CRC-32 of its trailer.  SMG_ENODEV without a device.                                  */
int smg_count_bgzf_inflate(const char *path, int32_t device, uint8_t **text, int64_t *n, double *ms_kernel, char *errbuf, size_t errlen);

/* host only: the stripped stream (see the top of this file) of inflated BAM text, fed to the framer of the counting calls
   in pieces of `piece` bytes (0: one piece), every record unpacked by the host routine that serves the records a piece
   boundary cuts.  *seq is malloc'ed (smg_count_free), *nseq its bytes.  SMG_EFORMAT, "<text>: BAM header: <reason>" or
   "<text>: BAM record at text offset <o>: <reason>" (o: where its block_size stands), for a negative l_text, n_ref, l_name
   or l_seq, a block_size smaller than 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq, and a text that ends inside
   the header or inside a record.                                                                                        */
int smg_count_bam_text(const uint8_t *text, int64_t n, int64_t piece, uint8_t **seq, int64_t *nseq, char *errbuf, size_t errlen);

/* the stripped stream of a whole BAM file by the route the counting calls take: inflated on `device`, framed on the host,
   unpacked on the device, the records a boundary between two inflate calls cuts from the host.  *seq is malloc'ed
   (smg_count_free), *nseq its bytes, *records (may be NULL) the contributing records, *ms_kernel (may be NULL) the sum of the
   HIP-event times of the unpack kernel alone.  SMG_EINVAL for a file that is not BAM, the errors of smg_count_bgzf_inflate
   with the path in place of <text> those of smg_count_bam_text.  SMG_ENODEV without a device.                            */
int smg_count_bam_strip(const char *path, int32_t device, uint8_t **seq, int64_t *nseq, int64_t *records, double *ms_kernel,
                        char *errbuf, size_t errlen);

/* host only: what the last call of this process that reads BAM (smg_count_files*, smg_count_bam_strip) read from the BAM
   file it was given as `path`: its contributing records, their bases, and in ms[4] (may be NULL) the milliseconds its reader
   thread spent on it: framing on the host (host clock), the inflate kernel, the unpack kernel (HIP events, summed over the
   launches), the copies of the stripped bytes to the host (host clock).  SMG_EINVAL where that call read no such BAM file to
   its end.                                                                                                              */
int smg_count_bam_report(const char *path, int64_t *records, int64_t *bases, double *ms);

/* the text of a whole gzip file (plain gzip, or BGZF read as such) by the route the counting calls take with the option on:
   the index of its restart points on `device`, then the exact decoder over it.  span_bytes: compressed bytes of a span,
   1024 .. 1048576, 0 for the default of 262144 (or the test hook SMG_COUNT_GZIP_SPAN).  *text is malloc'ed (smg_count_free),
   *n its bytes, ms_kernel[3] (may be NULL) the HIP-event times of the block finder with the marker decoder, of the resolver
   and of the exact decoder, summed over the launches.  SMG_EINVAL for a file that is not gzip and for the one refusal;
   SMG_EFORMAT "<path>: gzip member at offset <o>: <reason>" (header, trailer, CRC-32, ISIZE, truncation, trailing bytes that
   are neither zeros nor a member) or "<path>: deflate block at offset <o>: <reason>".  SMG_ENODEV without a device.     */
int smg_count_gzip_inflate(const char *path, int32_t device, int64_t span_bytes, uint8_t **text, int64_t *n, double *ms_kernel,
                           char *errbuf, size_t errlen);

/* host only: the same text by the same finder, marker decoder, chain, resolver and exact decoder, run as one lane on the host.
   A test twin like smg_count_bam_text, not a fallback of the counting calls.  Errors as smg_count_gzip_inflate.            */
int smg_count_gzip_text_host(const char *path, int64_t span_bytes, uint8_t **text, int64_t *n, char *errbuf, size_t errlen);

/* host only: what the last call of this process that reads plain gzip (a counting call with the option on,
   smg_count_gzip_inflate, smg_count_gzip_text_host) read of the file it was given as `path`: its members, its text bytes, the
   spans its pieces were cut into, how many decodes were linked (a span whose candidate is where the decode in front of it
   ended, the first of a piece included) and how many repaired (decoded again from a known end); every byte of text comes
   from one or the other.  ms[3] (may be NULL): as ms_kernel above (the twin: zeros).  Both routes give the same counts for
   the same file and span size.  SMG_EINVAL where that call read no such file.                                            */
int smg_count_gzip_report(const char *path, int64_t *members, int64_t *text_bytes, int64_t *spans, int64_t *linked, int64_t *repaired,
                          double *ms);

/* host only, plain files only: the records of a k-mer dump (see the top of this file) by the line decoder the kernel compiles,
   run on the host: per line, in line order, the canonical k-mer (*key_words left-aligned words) and the count saturated at
   2^32 - 1.  *keys (uint64[*n * *key_words]) and *counts (uint32[*n]) are malloc'ed (smg_count_free).  The errors of the
   counting calls with the dump option: SMG_EINVAL for a text that does not begin with a base, SMG_EFORMAT for the first bad
   line.  A test twin like smg_count_gzip_text_host, not a fallback.                                                       */
int smg_count_dump_parse(const char *path, int32_t kmer, uint64_t **keys, uint32_t **counts, int64_t *n, int *key_words,
                         char *errbuf, size_t errlen);

/* the same records as the kernel of the counting calls emits them, by the route those calls take (plain; BGZF; with gzip != 0
   plain gzip): in no particular order.  *ms_kernel (may be NULL): the sum of the HIP-event times of the line kernel.  Same
   errors.  SMG_ENODEV without a device.                                                                                */
int smg_count_dump_records(const char *path, int32_t kmer, int32_t device, int32_t gzip, uint64_t **keys, uint32_t **counts, int64_t *n,
                           int *key_words, double *ms_kernel, char *errbuf, size_t errlen);

void smg_count_free(void *p);
const char *smg_count_version(void);

#ifdef __cplusplus
}
#endif
#endif
