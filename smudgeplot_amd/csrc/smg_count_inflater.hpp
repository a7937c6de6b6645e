// smg_count_inflater.hpp -- the device stage of compressed input in front of the k-mer counter: the Inflater of the reader
// threads (smg_count_reader.hpp) on the device, one per thread, on a stream of its own, owning its buffers like the parts of
// smg_count_parts.hpp (smg_count.hip holds the map of the whole counter).
//   inflate   the members of a chunk, H2D -> inf_members (smg_inflate.hpp), one per wave -> statuses and text, D2H
//   unpack    for BAM: the descriptors, H2D -> bam_unpack (smg_bam.hpp) over the text where inflate left it, BAM_SLAB bytes
//             of output at a time -> D2H -> the sink
//   gzip      for plain gzip (smg_gzip.hpp): the first pass where the counter surveys its inputs (gzip_survey: the index of the
//             file), the second where its reader thread reads it (gzip_text), both through the DeviceGzEngine it owns
// and the BGZF file that one of the one-file routes opens for an inflater of its own.

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <map>
#include <memory>
#include <string>

#include "smg_count.h"
#include "smg_keysort.hpp"
#include "smg_count_err.hpp"
#include "smg_count_reader.hpp"
#include "smg_count_parts.hpp"
#include "smg_inflate.hpp"
#include "smg_bam.hpp"
#include "smg_gzip.hpp"

static_assert(sizeof(InfBlock) == sizeof(BgzfBlock) && sizeof(BgzfBlock) == 20, "the kernel reads the reader's blocks as they are");

#define BAM_SLAB     ((size_t) 32 << 20)                       // output bytes of one launch of bam_unpack (a multiple of BAM_TILE)
#define BAM_MAX_DESC (BGZF_TEXT / 36 + 1)                      // records that begin in the text of one call: 36 bytes each at least
static_assert(BAM_SLAB % BAM_TILE == 0, "a slab is whole tiles");

// a stream and the two events that time a kernel on it
struct TimedStream
{ hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  TimedStream() = default;
  TimedStream(const TimedStream &) = delete;
  TimedStream &operator=(const TimedStream &) = delete;
  ~TimedStream()
  { if (ev0) (void) hipEventDestroy(ev0);
    if (ev1) (void) hipEventDestroy(ev1);
    if (stream) (void) hipStreamDestroy(stream);
  }
  hipError_t init()
  { hipError_t e;
    if ((e = hipStreamCreate(&stream)) != hipSuccess) return e;
    if ((e = hipEventCreate(&ev0)) != hipSuccess) return e;
    return hipEventCreate(&ev1);
  }
};

// The four steps of plain gzip (smg_gzip.hpp) on the device, for the inflater that owns it: on its stream, the text of the
// second pass where the inflater's BGZF text goes.  It owns the piece (pinned and on the device), the ring slots of the
// first pass, and the windows of the restart points of every file it indexed, in slabs, until it goes.
#define GZ_SLAB 512                                            // windows of a slab
struct DeviceGzEngine : GzEngine
{ int device;
  TimedStream &q;
  uint8_t *d_text, *h_text;                                    // the inflater's, BGZF_TEXT bytes each
  Pinned<uint8_t> h_piece;
  Pinned<GzTask> h_tasks;
  Pinned<GzResult> h_res;
  Pinned<GzCheck> h_check;
  Pinned<GzExact> h_iv;
  Pinned<uint32_t> h_word;                                     // CRCs, then statuses, of the exact decoder; [0]: the resolver's flag
  DevBuf<uint8_t> d_piece;
  DevBuf<uint16_t> d_rings;
  DevBuf<GzCheck> d_check;
  DevBuf<GzTask> d_tasks;
  DevBuf<GzResult> d_spec, d_rep;
  DevBuf<GzExact> d_iv;
  DevBuf<uint32_t> d_word, d_bad;
  std::vector<std::unique_ptr<DevBuf<uint8_t>>> slabs;
  std::vector<hipEvent_t> ev;                                  // pairs around the launches of the resolver since the last resolved()
  size_t ev_used = 0;
  int64_t nwin = 0;
  size_t piece_n = 0;
  uint32_t nspec = 0;

  DeviceGzEngine(int dev, TimedStream &stream, uint8_t *dt, uint8_t *ht) : device(dev), q(stream), d_text(dt), h_text(ht) {}
  ~DeviceGzEngine() override { for (hipEvent_t e : ev) (void) hipEventDestroy(e); }

  hipError_t init()
  { hipError_t e;
    const size_t ntask = GZ_MAX_SPANS + 2;
    if ((e = h_piece.alloc(GZ_MAX_PIECE)) != hipSuccess) return e;
    if ((e = h_tasks.alloc(sizeof(GzTask) * ntask)) != hipSuccess) return e;
    if ((e = h_res.alloc(sizeof(GzResult) * ntask)) != hipSuccess) return e;
    if ((e = h_check.alloc(sizeof(GzCheck) * GZ_SLOTS)) != hipSuccess) return e;
    if ((e = h_iv.alloc(sizeof(GzExact) * GZ_MAX_EXACT)) != hipSuccess) return e;
    if ((e = h_word.alloc(sizeof(uint32_t) * 2 * GZ_MAX_EXACT)) != hipSuccess) return e;
    if ((e = d_piece.alloc(GZ_MAX_PIECE)) != hipSuccess) return e;
    if ((e = d_rings.alloc(sizeof(uint16_t) * INF_WINDOW * (size_t) GZ_SLOTS)) != hipSuccess) return e;
    if ((e = d_check.alloc(sizeof(GzCheck) * GZ_SLOTS)) != hipSuccess) return e;
    if ((e = d_tasks.alloc(sizeof(GzTask) * ntask)) != hipSuccess) return e;
    if ((e = d_spec.alloc(sizeof(GzResult) * ntask)) != hipSuccess) return e;
    if ((e = d_rep.alloc(sizeof(GzResult) * ntask)) != hipSuccess) return e;
    if ((e = d_iv.alloc(sizeof(GzExact) * GZ_MAX_EXACT)) != hipSuccess) return e;
    if ((e = d_word.alloc(sizeof(uint32_t) * 2 * GZ_MAX_EXACT)) != hipSuccess) return e;
    if ((e = d_bad.alloc(sizeof(uint32_t))) != hipSuccess) return e;
    return hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), q.stream);
  }

  uint8_t *piece_buf(size_t n) override { return n <= GZ_MAX_PIECE ? (uint8_t *) h_piece : nullptr; }
  int piece(size_t n) override
  { const Errors x{ errbuf, errlen };
    DCHK(hipSetDevice(device));
    if (n) DCHK(hipMemcpyAsync(d_piece, h_piece, n, hipMemcpyHostToDevice, q.stream));
    piece_n = n;
    return 0;
  }
  int marker(const GzTask *tasks, int n, bool spec, GzResult *res, GzCheck *check) override
  { const Errors x{ errbuf, errlen };
    if (n < 1 || n > GZ_MAX_SPANS + 2 || (!spec && n != 1)) return fail(errbuf, errlen, SMG_EINVAL, "internal error: %d gzip tasks in one launch", n);
    const size_t slot0 = spec ? 0 : (size_t) GZ_MAX_SPANS * GZ_QUOTA, nslot = spec ? (size_t) n * GZ_QUOTA : (size_t) GZ_REPAIR_QUOTA;
    if (slot0 + nslot > GZ_SLOTS) return fail(errbuf, errlen, SMG_EINVAL, "internal error: %zu gzip ring slots in one launch", slot0 + nslot);
    float t = 0;
    DCHK(hipSetDevice(device));
    memcpy(h_tasks, tasks, sizeof(GzTask) * (size_t) n);
    DCHK(hipMemcpyAsync(d_tasks, h_tasks, sizeof(GzTask) * (size_t) n, hipMemcpyHostToDevice, q.stream));
    GzResult *d_res = spec ? d_spec : d_rep;
    DCHK(hipEventRecord(q.ev0, q.stream));
    hipLaunchKernelGGL(gz_marker_k, dim3((unsigned) n), dim3(64), 0, q.stream, d_piece, (uint32_t) piece_n, d_tasks, n, d_spec, spec ? 0u : nspec, span,
                       check_text, d_rings, d_check, d_res);
    DCHK(hipGetLastError());
    DCHK(hipEventRecord(q.ev1, q.stream));
    DCHK(hipMemcpyAsync(h_res, d_res, sizeof(GzResult) * (size_t) n, hipMemcpyDeviceToHost, q.stream));
    DCHK(hipMemcpyAsync(h_check, d_check + slot0, sizeof(GzCheck) * nslot, hipMemcpyDeviceToHost, q.stream));
    DCHK(hipStreamSynchronize(q.stream));
    DCHK(hipEventElapsedTime(&t, q.ev0, q.ev1));
    ms[0] += t;
    memcpy(res, h_res, sizeof(GzResult) * (size_t) n);
    memcpy(check, h_check, sizeof(GzCheck) * nslot);
    if (spec) nspec = (uint32_t) n;
    return 0;
  }
  int64_t windows(int n) override
  { if (n < 1 || n > GZ_SLAB) return -1;
    if (nwin % GZ_SLAB + n > GZ_SLAB) nwin = (nwin / GZ_SLAB + 1) * GZ_SLAB;       // (those of one decode are neighbours)
    while ((int64_t) slabs.size() * GZ_SLAB < nwin + n)
      { if (hipSetDevice(device) != hipSuccess) return -1;
        std::unique_ptr<DevBuf<uint8_t>> s(new DevBuf<uint8_t>());
        if (s->alloc((size_t) GZ_SLAB * INF_WINDOW) != hipSuccess) return -1;
        slabs.push_back(std::move(s));
      }
    const int64_t w0 = nwin;
    nwin += n;
    return w0;
  }
  uint8_t *window(int64_t w) override { return (uint8_t *) *slabs[(size_t) (w / GZ_SLAB)] + (size_t) (w % GZ_SLAB) * INF_WINDOW; }
  int resolve(uint32_t slot0, uint32_t ncheck, uint64_t end_text, int64_t prev, uint32_t prev_avail, int64_t dst) override
  { const Errors x{ errbuf, errlen };
    DCHK(hipSetDevice(device));
    if (ev_used + 2 > ev.size())
      for (int i = 0; i < 2; i++)
        { hipEvent_t e = nullptr;
          DCHK(hipEventCreate(&e));
          ev.push_back(e);
        }
    DCHK(hipEventRecord(ev[ev_used], q.stream));
    hipLaunchKernelGGL(gz_resolve_k, dim3(ncheck + 1), dim3(256), 0, q.stream, d_rings, d_check, slot0, ncheck, end_text,
                       prev < 0 ? (const uint8_t *) nullptr : window(prev), prev_avail, window(dst), d_bad);
    DCHK(hipGetLastError());
    DCHK(hipEventRecord(ev[ev_used + 1], q.stream));
    ev_used += 2;
    return 0;
  }
  int resolved(bool *bad) override
  { const Errors x{ errbuf, errlen };
    DCHK(hipSetDevice(device));
    DCHK(hipMemcpyAsync(h_word, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, q.stream));
    DCHK(hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), q.stream));
    DCHK(hipStreamSynchronize(q.stream));
    for (size_t i = 0; i + 1 < ev_used; i += 2)
      { float t = 0;
        DCHK(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
        ms[1] += t;
      }
    ev_used = 0;
    *bad = h_word[0] != 0;
    return 0;
  }
  int exact(const GzExact *iv, int n, size_t text_n, const uint8_t **text, uint32_t *crc, uint32_t *status) override
  { const Errors x{ errbuf, errlen };
    if (n < 1 || n > GZ_MAX_EXACT || text_n > BGZF_TEXT)
      return fail(errbuf, errlen, SMG_EINVAL, "internal error: %d gzip intervals with %zu bytes of text in one launch", n, text_n);
    float t = 0;
    DCHK(hipSetDevice(device));
    memcpy(h_iv, iv, sizeof(GzExact) * (size_t) n);
    DCHK(hipMemcpyAsync(d_iv, h_iv, sizeof(GzExact) * (size_t) n, hipMemcpyHostToDevice, q.stream));
    DCHK(hipEventRecord(q.ev0, q.stream));
    hipLaunchKernelGGL(gz_exact_k, dim3((unsigned) n), dim3(64), 0, q.stream, d_piece, (uint32_t) piece_n, d_iv, n, d_text, (uint32_t) text_n, d_word,
                       d_word + GZ_MAX_EXACT);
    DCHK(hipGetLastError());
    DCHK(hipEventRecord(q.ev1, q.stream));
    DCHK(hipMemcpyAsync(h_word, d_word, sizeof(uint32_t) * 2 * GZ_MAX_EXACT, hipMemcpyDeviceToHost, q.stream));
    if (text_n) DCHK(hipMemcpyAsync(h_text, d_text, text_n, hipMemcpyDeviceToHost, q.stream));
    DCHK(hipStreamSynchronize(q.stream));
    DCHK(hipEventElapsedTime(&t, q.ev0, q.ev1));
    ms[2] += t;
    memcpy(crc, h_word, sizeof(uint32_t) * (size_t) n);
    memcpy(status, h_word + GZ_MAX_EXACT, sizeof(uint32_t) * (size_t) n);
    *text = h_text;
    return 0;
  }
  void reset() override { slabs.clear(); nwin = 0; }
};

struct DeviceInflater : Inflater
{ int device = 0;
  TimedStream q;
  // (declared in the order they are allocated, hence freed in the reverse of it, as they always were)
  Pinned<uint8_t> h_chunk;                                     // the base's chunk and blk
  Pinned<BgzfBlock> h_blk;
  Pinned<uint8_t> h_text;
  Pinned<uint32_t> h_status;
  DevBuf<uint8_t> d_chunk;
  DevBuf<InfBlock> d_blk;
  DevBuf<uint8_t> d_text;
  DevBuf<uint32_t> d_status;
  // the second step, for BAM: set up by the first piece that needs it (a file shows that it is BAM only in its text)
  Pinned<BamDesc> h_desc;
  Pinned<uint8_t> h_out;
  DevBuf<BamDesc> d_desc;
  DevBuf<uint8_t> d_out;
  size_t text_n = 0;                                           // text bytes of the last inflate call
  InflaterTimes ms;                                            // the two kernels (HIP events); the copies of unpack's output (host clock)
  // plain gzip: set up by the first such file the survey of a call that opted in meets; the index of every file by its path
  std::unique_ptr<DeviceGzEngine> gz;
  std::map<std::string, GzIndex> gz_index;

  // pinned and device memory for a chunk, its blocks, their text and statuses; 0 or the HIP error
  hipError_t init(int dev)
  { device = dev;
    hipError_t e;
    if ((e = hipSetDevice(dev)) != hipSuccess) return e;
    if ((e = q.init()) != hipSuccess) return e;
    if ((e = h_chunk.alloc(SMG_COUNT_BGZF_CHUNK)) != hipSuccess) return e;
    if ((e = h_blk.alloc(sizeof(BgzfBlock) * BGZF_MAX_BLOCKS)) != hipSuccess) return e;
    chunk = h_chunk; blk = h_blk;
    if ((e = h_text.alloc(BGZF_TEXT)) != hipSuccess) return e;
    if ((e = h_status.alloc(sizeof(uint32_t) * BGZF_MAX_BLOCKS)) != hipSuccess) return e;
    if ((e = d_chunk.alloc(SMG_COUNT_BGZF_CHUNK)) != hipSuccess) return e;
    if ((e = d_blk.alloc(sizeof(InfBlock) * BGZF_MAX_BLOCKS)) != hipSuccess) return e;
    if ((e = d_text.alloc(BGZF_TEXT)) != hipSuccess) return e;
    return d_status.alloc(sizeof(uint32_t) * BGZF_MAX_BLOCKS);
  }

  const char *reason(int status) const override { return inflate_reason(status); }
  InflaterTimes times() const override { return ms; }

  // The first pass over a plain gzip file (smg_gzip.hpp), where the counter surveys its inputs: the index of its restart
  // points stays here under its path, *text_bytes = its text, exactly.  span_bytes: 0 for the default (or the test hook)
  int gzip_survey(int fd, const char *path, int64_t span_bytes, int64_t *text_bytes, char *errbuf, size_t errlen)
  { uint32_t span = 0;
    RCHK(gz_span(span_bytes, &span, errbuf, errlen));
    if (!gz)
      { std::unique_ptr<DeviceGzEngine> e(new DeviceGzEngine(device, q, d_text, h_text));
        hipError_t he = hipSetDevice(device);
        if (he == hipSuccess) he = e->init();
        if (he != hipSuccess)
          return fail(errbuf, errlen, he == hipErrorOutOfMemory ? SMG_ENOMEM : SMG_ENODEV, "cannot set up the gzip inflater: %s", hipGetErrorString(he));
        gz.swap(e);
      }
    gz->set_span(span);
    GzIndex &ix = gz_index[path];
    const int rc = gz_build(fd, path, *gz, ix, BGZF_TEXT, GZ_MAX_PIECE, errbuf, errlen);
    if (rc) { gz_index.erase(path); return rc; }
    *text_bytes = ix.text;
    return 0;
  }
  bool has_gzip(const char *path) const override { return gz && gz_index.count(path) != 0; }
  // the second pass: as many restart intervals a launch as fit BGZF_TEXT, their text where BGZF text goes
  int gzip_text(int fd, const char *path, const std::function<int(const uint8_t *, size_t)> &put, char *errbuf, size_t errlen) override
  { const auto it = gz_index.find(path);
    if (!gz || it == gz_index.end()) return Inflater::gzip_text(fd, path, put, errbuf, errlen);
    text_n = 0;
    return gz_feed(fd, path, *gz, it->second, BGZF_TEXT, GZ_MAX_PIECE, put, errbuf, errlen);
  }

  // H2D of the members, the kernel, D2H of statuses and text.  The reader has bounded every block: its payload lies
  // in the chunk, its text in BGZF_TEXT bytes, and the kernel stays inside both whatever the payload says.
  int inflate(int n, const uint8_t **text, int *bad, char *errbuf, size_t errlen) override
  { const Errors x{ errbuf, errlen };
    size_t in_end = 0, out_end = 0;
    for (int i = 0; i < n; i++)
      { const size_t ie = (size_t) blk[i].in_off + blk[i].clen, oe = (size_t) blk[i].out_off + blk[i].isize;
        if (ie > in_end) in_end = ie;
        if (oe > out_end) out_end = oe;
      }
    if (n < 1 || n > BGZF_MAX_BLOCKS || in_end > (size_t) SMG_COUNT_BGZF_CHUNK || out_end > BGZF_TEXT)
      return fail(errbuf, errlen, SMG_EINVAL, "internal error: %d BGZF blocks of %zu bytes with %zu bytes of text in one launch", n, in_end, out_end);
    float t = 0;
    DCHK(hipSetDevice(device));                                // (a reader thread has not chosen its device yet)
    DCHK(hipMemcpyAsync(d_chunk, chunk, in_end, hipMemcpyHostToDevice, q.stream));
    DCHK(hipMemcpyAsync(d_blk, blk, sizeof(InfBlock) * (size_t) n, hipMemcpyHostToDevice, q.stream));
    DCHK(hipEventRecord(q.ev0, q.stream));
    hipLaunchKernelGGL(inf_members, dim3((unsigned) n), dim3(64), 0, q.stream, d_chunk, d_blk, n, d_text, d_status);
    DCHK(hipGetLastError());
    DCHK(hipEventRecord(q.ev1, q.stream));
    DCHK(hipMemcpyAsync(h_status, d_status, sizeof(uint32_t) * (size_t) n, hipMemcpyDeviceToHost, q.stream));
    if (out_end) DCHK(hipMemcpyAsync(h_text, d_text, out_end, hipMemcpyDeviceToHost, q.stream));
    DCHK(hipStreamSynchronize(q.stream));
    DCHK(hipEventElapsedTime(&t, q.ev0, q.ev1));
    ms.inflate += t;
    text_n = 0;
    for (int i = 0; i < n; i++)
      if (h_status[i] != INF_OK) { *bad = i; return h_status[i] < INF_NSTATUS ? (int) h_status[i] : INF_NSTATUS; }
    *text = h_text;
    text_n = out_end;
    return 0;
  }

  // H2D of the descriptors, then BAM_SLAB bytes of output at a time: bam_unpack over their tiles, D2H into pinned memory,
  // the sink.  The descriptors are checked against the text and the output here, and the kernel stays inside both anyway.
  int unpack(const BamDesc *d, size_t nd, size_t out_len, Sink &sink, char *errbuf, size_t errlen) override
  { const Errors x{ errbuf, errlen };
    if (nd > BAM_MAX_DESC || out_len > 0xFFFFFFFFu - 2 * BAM_SLAB || !bam_desc_ok(d, nd, text_n, out_len))
      return fail(errbuf, errlen, SMG_EINVAL, "internal error: %zu BAM records with %zu bases do not describe a text of %zu bytes", nd, out_len, text_n);
    if (out_len == 0) return 0;
    DCHK(hipSetDevice(device));
    if (!d_out)
      { DCHK(h_desc.alloc(sizeof(BamDesc) * BAM_MAX_DESC));
        DCHK(h_out.alloc(BAM_SLAB));
        DCHK(d_desc.alloc(sizeof(BamDesc) * BAM_MAX_DESC));
        DCHK(d_out.alloc(BAM_SLAB));
      }
    memcpy(h_desc, d, sizeof(BamDesc) * nd);
    DCHK(hipMemcpyAsync(d_desc, h_desc, sizeof(BamDesc) * nd, hipMemcpyHostToDevice, q.stream));
    for (size_t base = 0; base < out_len; base += BAM_SLAB)
      { const size_t len = out_len - base < BAM_SLAB ? out_len - base : BAM_SLAB;
        float t = 0;
        DCHK(hipEventRecord(q.ev0, q.stream));
        hipLaunchKernelGGL(bam_unpack, dim3((unsigned) ((len + BAM_TILE - 1) / BAM_TILE)), dim3(BAM_LANES), 0, q.stream, d_text, (uint32_t) text_n,
                           d_desc, (uint32_t) nd, d_out, (uint32_t) base, (uint32_t) len);
        DCHK(hipGetLastError());
        DCHK(hipEventRecord(q.ev1, q.stream));
        DCHK(hipStreamSynchronize(q.stream));
        DCHK(hipEventElapsedTime(&t, q.ev0, q.ev1));
        ms.unpack += t;
        const double t0 = now_ms();
        DCHK(hipMemcpyAsync(h_out, d_out, len, hipMemcpyDeviceToHost, q.stream));
        DCHK(hipStreamSynchronize(q.stream));
        ms.d2h += now_ms() - t0;
        if (!sink.put(h_out, len)) return 1;
      }
    return 0;
  }
};

// a device inflater, or the error
static int new_inflater(int device, std::unique_ptr<DeviceInflater> &out, char *errbuf, size_t errlen)
{ RCHK(check_device(device, errbuf, errlen));
  out.reset(new DeviceInflater());
  const hipError_t e = out->init(device);
  if (e != hipSuccess)
    return fail(errbuf, errlen, e == hipErrorOutOfMemory ? SMG_ENOMEM : SMG_ENODEV, "cannot set up the BGZF inflater: %s", hipGetErrorString(e));
  return 0;
}

// A BGZF file opened for an inflater of its own, for the routes that read one file: scanned (what is not BGZF is refused),
// its text bytes known, then the inflater, then the file.
struct BgzfInput
{ int64_t blocks = 0, text_bytes = 0;
  std::unique_ptr<DeviceInflater> infl;
  std::unique_ptr<Fd> file;
  Source src;                                                  // (a file: the scan refuses a stream)

  int open(const char *path, int device, char *errbuf, size_t errlen)
  { RCHK(bgzf_scan(path, &blocks, &text_bytes, errbuf, errlen));
    RCHK(new_inflater(device, infl, errbuf, errlen));
    file.reset(new Fd(path));
    if (file->fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", path);
    src = Source(file->fd, false);
    return 0;
  }
};
