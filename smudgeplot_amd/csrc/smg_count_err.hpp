// smg_count_err.hpp -- how every part of the k-mer counter reports an error: the message into the caller's buffer, the
// code as the return value.  Host only.

#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdio>

static inline int fail(char *errbuf, size_t errlen, int code, const char *fmt, ...)
{ if (errbuf && errlen)
    { va_list ap;
      va_start(ap, fmt);
      vsnprintf(errbuf, errlen, fmt, ap);
      va_end(ap);
    }
  return code;
}
