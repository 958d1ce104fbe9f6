// prv_buffer.hpp -- who owns what on the host side of the C ABI (prv_api.cpp and its *_api.inc files):
//   Buffer      a block of device memory, freed by its destructor;
//   BufferPool  the blocks destroyed trainers leave to their context, taken again by size;
//   ensure      the grow-only allocation every workspace goes through;
//   PinnedStage the pinned host block a context builds its per-call camera upload in, and the event that guards it;
//   Handle      the base of every object a context hands out (trainer, communicator, mesh, index, coverage handle): the
//               context keeps one list of them and makes them inert when it goes first.
// Host code only, and nothing of HIP but the runtime calls made here: tests/test_buffers_host.py compiles this file into a
// stand-alone program against counting stubs of those calls.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <utility>
#include <vector>

namespace prv {

// bytes held by the live Buffers of the process (prv_debug_live_bytes): up in ensure, down where a block is freed; a move
// takes its bytes along
inline std::atomic<unsigned long long> g_live_buffer_bytes{0};

struct Buffer {
  void* p = nullptr;
  size_t bytes = 0;

  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  Buffer(Buffer&& o) noexcept : p(o.p), bytes(o.bytes) {
    o.p = nullptr;
    o.bytes = 0;
  }
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p;
      bytes = o.bytes;
      o.p = nullptr;
      o.bytes = 0;
    }
    return *this;
  }
  ~Buffer() { reset(); }

  // an empty buffer makes no runtime call: a handle emptied when its context went may be deleted after the device was reset
  void reset() { (void)free_block(); }
  hipError_t free_block() { // reset(), for the one caller that reports the runtime's answer
    if (!p) return hipSuccess;
    const hipError_t e = hipFree(p);
    g_live_buffer_bytes.fetch_sub(bytes);
    p = nullptr;
    bytes = 0;
    return e;
  }
};

// Parked memory is bounded (16 GiB of the device's 288, 512 buffers); the oldest go first, so sizes nobody asks for any more
// do not stay for the life of the context.
struct BufferPool {
  static constexpr size_t kMaxBytes = (size_t)16 << 30, kMaxCount = 512;
  std::vector<Buffer> idle; // oldest first
  size_t bytes = 0;

  void park(Buffer&& b) { // b ends empty either way
    Buffer in(std::move(b));
    if (!in.p || in.bytes > kMaxBytes) return;
    while (!idle.empty() && (idle.size() >= kMaxCount || bytes + in.bytes > kMaxBytes)) {
      bytes -= idle.front().bytes;
      idle.erase(idle.begin());
    }
    bytes += in.bytes;
    idle.push_back(std::move(in));
  }
  bool take(Buffer& b, size_t want) { // the oldest block of exactly `want` bytes
    for (size_t i = 0; i < idle.size(); i++)
      if (idle[i].bytes == want) {
        b = std::move(idle[i]);
        bytes -= want;
        idle.erase(idle.begin() + (long)i);
        return true;
      }
    return false;
  }
  void clear() {
    idle.clear();
    bytes = 0;
  }
};

// b holds at least `bytes` afterwards.  Grows only; the stream is synchronised before the old block is freed; when the
// device is out of memory the context's parked blocks go before anybody fails; after a failed allocation b.p is null.
// *call names the runtime call that failed, as the error text of the ABI spells it.
inline hipError_t ensure(Buffer& b, size_t bytes, hipStream_t stream, BufferPool& parked, const char** call) {
  if (b.bytes >= bytes && b.p) return hipSuccess;
  hipError_t e;
  if (b.p) {
    *call = "hipStreamSynchronize(c->stream)";
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    *call = "hipFree(b.p)";
    if ((e = b.free_block()) != hipSuccess) return e;
  }
  void* p = nullptr;
  e = hipMalloc(&p, bytes);
  if (e == hipErrorOutOfMemory && !parked.idle.empty()) {
    (void)hipGetLastError();
    *call = "hipStreamSynchronize(c->stream)";
    const hipError_t s = hipStreamSynchronize(stream);
    if (s != hipSuccess) return s;
    parked.clear();
    e = hipMalloc(&p, bytes);
  }
  *call = "e";
  if (e != hipSuccess) return e;
  b.p = p;
  b.bytes = bytes;
  g_live_buffer_bytes.fetch_add(bytes);
  return hipSuccess;
}

// The pinned host block that small per-call uploads are built in and sent from: no pageable copy, and the host never waits
// for the stream.  What makes that safe is in these two functions and nowhere else: send() records an event behind its copy,
// and acquire() waits for that event before it hands the block out to be rewritten (or frees it to grow).  An acquire that no
// send follows -- the caller returned early -- leaves nothing to wait for.  *call names the runtime call that failed, as the
// error text of the ABI spells it.
struct PinnedStage {
  static constexpr size_t kMinBytes = 8192;
  void* p = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr; // created on first use, timing disabled
  bool in_flight = false;  // ev was recorded behind a copy out of p and has not been waited for since

  PinnedStage() = default;
  PinnedStage(const PinnedStage&) = delete;
  PinnedStage& operator=(const PinnedStage&) = delete;
  PinnedStage(PinnedStage&& o) noexcept : p(o.p), cap(o.cap), ev(o.ev), in_flight(o.in_flight) { o.forget(); }
  PinnedStage& operator=(PinnedStage&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap, ev = o.ev, in_flight = o.in_flight;
      o.forget();
    }
    return *this;
  }
  ~PinnedStage() { release(); }

  // *out = the block, at least `bytes`, free to be written.  After a refused allocation the stage is empty and may be used again
  hipError_t acquire(size_t bytes, void** out, const char** call) {
    hipError_t e;
    if (in_flight) {
      *call = "hipEventSynchronize(c->pin_ev)";
      if ((e = hipEventSynchronize(ev)) != hipSuccess) return e;
      in_flight = false;
    }
    if (cap < bytes) {
      if (p) (void)hipHostFree(p);
      p = nullptr;
      cap = 0;
      const size_t want = std::max(bytes, kMinBytes);
      *call = "hipHostMalloc(&c->pin, std::max<size_t>(up_bytes, 8192), hipHostMallocDefault)";
      if ((e = hipHostMalloc(&p, want, hipHostMallocDefault)) != hipSuccess) {
        p = nullptr;
        return e;
      }
      cap = want;
    }
    if (!ev) {
      *call = "hipEventCreateWithFlags(&c->pin_ev, hipEventDisableTiming)";
      if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) {
        ev = nullptr;
        return e;
      }
    }
    *out = p;
    return hipSuccess;
  }
  // the first `bytes` of the block to `dst` on `stream`, one asynchronous copy; the block is not to be written before the next acquire
  hipError_t send(void* dst, size_t bytes, hipStream_t stream, const char** call) {
    *call = "hipMemcpyAsync(c->view_ids.p, c->pin, up_bytes, hipMemcpyHostToDevice, c->stream)";
    hipError_t e = hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    *call = "hipEventRecord(c->pin_ev, c->stream)";
    if ((e = hipEventRecord(ev, stream)) == hipSuccess) in_flight = true;
    return e;
  }
  // frees the block and the event without waiting: the owner has drained the stream (prv_destroy does, first of all).  An empty
  // stage makes no runtime call
  void release() {
    if (p) (void)hipHostFree(p);
    if (ev) (void)hipEventDestroy(ev);
    forget();
  }

private:
  void forget() {
    p = nullptr;
    cap = 0;
    ev = nullptr;
    in_flight = false;
  }
};

// An object a context hands out.  Ctx has `device`, `stream` and `std::vector<Handle<Ctx>*> handles`.  A handle is in its
// context's list from construction to destruction, so a create function that returns early has nothing to undo.
template <class Ctx> struct Handle {
  Ctx* ctx; // null: the context was destroyed, the handle is inert (every entry point refuses it, destroying it is safe)

  explicit Handle(Ctx* c) : ctx(c) { c->handles.push_back(this); }
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  virtual ~Handle() {
    if (ctx) ctx->handles.erase(std::remove(ctx->handles.begin(), ctx->handles.end(), this), ctx->handles.end());
  }
  // gives up everything that lives on the device or needs the runtime; what is left makes no runtime call when it is deleted
  virtual void detach() = 0;
  // last words of a handle destroyed while its context lives (device current, context stream drained): the trainer parks here
  virtual void retire() {}
};

// the context goes first: its handles stay valid objects that own nothing
template <class Ctx> void detach_handles(Ctx* c) {
  for (Handle<Ctx>* h : c->handles) {
    h->detach();
    h->ctx = nullptr;
  }
  c->handles.clear();
}

// every prv_*_destroy of a handle
template <class H> void destroy_handle(H* h) {
  if (!h) return;
  if (h->ctx) {
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    h->retire();
  }
  delete h;
}

} // namespace prv
