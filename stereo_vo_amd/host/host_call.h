// What every synchronous host entry shares and needs no GPU for ("the synchronous entries share one sequence"): how a
// refusal of a host/*_args.h check goes into the context, the order of the steps around a _dev entry, and the layout of the one
// temporary device buffer.  csrc/common.h binds the sequence to HIP (svo_host_call, SvoTemp); tests/sanitize/host_call_test.cpp
// walks every combination of failures and the carver on a CPU.
#ifndef SVO_HOST_CALL_H_
#define SVO_HOST_CALL_H_
#include <stddef.h>

// How an entry stores a refusal in its context: `call` is one of the host/*.h checks with `&err` as its last argument.
#define SVO_ARGS_CHECK(ctx, call) do { const char* err = nullptr; if (call) { (ctx)->err = err; return SVO_ERR_INVALID; } } while (0)

// The steps of a synchronous entry around its _dev entry.  `e_up` is the error the copies up left; `dev` runs the _dev entry, only
// if they succeeded; `back` queues the copies down, only if `dev` ran and returned 0; `drain` waits for the stream exactly once and
// after both, whatever failed, so that the caller's temporary buffer may go away.  A non-zero `dev` result is returned as it is (its
// message stands).  Otherwise 0 is returned with *failed the first failing error of (up, back, drain), or Err() when none failed.
template <typename Err, typename Dev, typename Back, typename Drain>
inline int svo_host_sequence(Err e_up, Dev dev, Back back, Drain drain, Err* failed) {
  const Err ok = Err();
  Err e = e_up;
  const int rc = e == ok ? dev() : 0;
  if (e == ok && !rc) e = back();
  const Err e_drain = drain();
  *failed = e == ok ? e_drain : e;
  return rc;
}

// The layout of a temporary buffer: add() gives the next part's offset, a multiple of 256 bytes (SvoScratch's rounding and
// hipMalloc's alignment, beyond what any _dev check asks for); a part of 0 bytes takes no room; total() is the buffer's size.
struct SvoParts {
  size_t add(size_t bytes) {
    const size_t at = (end_ + 255) & ~(size_t)255;
    if (bytes) end_ = at + bytes;
    return at;
  }
  size_t total() const { return end_; }
 private:
  size_t end_ = 0;
};
#endif  // SVO_HOST_CALL_H_
