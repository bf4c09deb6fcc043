// What the host sides of the device codecs share (csrc/jpeg_plan.h, csrc/png_plan.h, the entry points of the two .hip files): how a
// refusal becomes the entry point's error, and the check of a caller's buffers.  Plain C++, no HIP: tests/native builds it too.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

void vqn_set_error(const char* fmt, ...);  // csrc/error.cpp (only codec_refuse needs it: the stand-alone programs do not link it)

// check(why, len) -> 0, or -1 (bad argument) / -2 (unsupported shape) with its reason in why: a planner or a buffer check with its
// arguments bound.  -> 0, or the reason under the name `fn` as the library's error and the same -1 / -2: VQN_EARG / VQN_ESHAPE.
template <typename Check>
inline int codec_refuse(const char* fn, Check check) {
  char why[256];
  const int rc = check(why, sizeof(why));
  if (rc == 0) return 0;
  vqn_set_error("%s: %s", fn, why);
  return rc == -2 ? -2 : -1;
}

// The buffers a caller hands to an encoder against its plan -> 0, or -1 with the reason in msg.  first_only: the first kernel alone
// runs, which needs scratch_first bytes of the scratch and no output.
inline int codec_check_buffers(int64_t scratch_first, int64_t scratch_all, int64_t out_all, int64_t scratch_bytes, int64_t out_bytes,
                               int first_only, char* msg, size_t msg_len) {
  const int64_t need = first_only ? scratch_first : scratch_all;
  if (scratch_bytes < need) {
    snprintf(msg, msg_len, "bad argument: the scratch holds %lld bytes, the batch needs %lld", (long long)scratch_bytes, (long long)need);
    return -1;
  }
  if (!first_only && out_bytes < out_all) {
    snprintf(msg, msg_len, "bad argument: a byte total of up to %lld over the buffer of %lld bytes", (long long)out_all,
             (long long)out_bytes);
    return -1;
  }
  return 0;
}
