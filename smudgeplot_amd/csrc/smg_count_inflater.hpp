// smg_count_inflater.hpp -- the device stage of compressed input in front of the k-mer counter: the Inflater of the reader
// threads (smg_count_reader.hpp) on the device, one per thread, on a stream of its own, owning its buffers like the parts of
// smg_count_parts.hpp (smg_count.hip holds the map of the whole counter).
//   inflate   the members of a chunk, H2D -> inf_members (smg_inflate.hpp), one per wave -> statuses and text, D2H
//   unpack    for BAM: the descriptors, H2D -> bam_unpack (smg_bam.hpp) over the text where inflate left it, BAM_SLAB bytes
//             of output at a time -> D2H -> the sink
// and the BGZF file that one of the one-file routes opens for an inflater of its own.

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <memory>

#include "smg_count.h"
#include "smg_keysort.hpp"
#include "smg_count_err.hpp"
#include "smg_count_reader.hpp"
#include "smg_count_parts.hpp"
#include "smg_inflate.hpp"
#include "smg_bam.hpp"

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

  int open(const char *path, int device, char *errbuf, size_t errlen)
  { RCHK(bgzf_scan(path, &blocks, &text_bytes, errbuf, errlen));
    RCHK(new_inflater(device, infl, errbuf, errlen));
    file.reset(new Fd(path));
    if (file->fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", path);
    return 0;
  }
};
