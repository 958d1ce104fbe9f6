"""The C ABI's owners of device memory and of context-owned handles (nerf_prv_amd/csrc/prv_buffer.hpp) against a counting
stub of the runtime calls they make: every block is freed exactly once -- at scope exit, across moves, when a buffer grows,
on the out-of-memory path, through the parked pool, whichever of a handle and its context goes first, and on an early return
out of a create function.  The pinned upload staging (PinnedStage) likewise, and its protocol call for call: it waits for its
event exactly when a copy out of it may be in flight, and before it frees.  Host code only: a stand-alone program built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

PROGRAM = r"""
#include "prv_buffer.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <string>
using namespace prv;

// ---- the counting stub: every block is a heap block, so a double free or a leak is also the sanitizer's finding.  The log
// holds one letter per call: M hipMalloc, m a refused hipMalloc, F hipFree, S hipStreamSynchronize, D hipSetDevice, L hipGetLastError,
// H hipHostMalloc, h a refused hipHostMalloc, f hipHostFree, E hipEventCreateWithFlags, W hipEventSynchronize, R hipEventRecord,
// X hipEventDestroy, C hipMemcpyAsync.  A pinned block has its real size and the copy is made, so the sanitizer sees both ends
static std::string calls;
static std::set<void*> live;
static int n_malloc, n_free, refuse_next;
static bool frozen; // no runtime call may be made (the device has been reset)
static hipStream_t const STREAM = (hipStream_t)0x20;
static void call(char what) {
  if (frozen) { printf("runtime call '%c' after the context's end\n", what); exit(5); }
  calls += what;
}
extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
  if (refuse_next > 0) { refuse_next--; call('m'); *p = nullptr; return hipErrorOutOfMemory; }
  call('M');
  n_malloc++;
  *p = malloc(8); // (the size is the caller's book-keeping: 16 GiB buffers cost 8 bytes here)
  live.insert(*p);
  (void)bytes;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  call('F');
  n_free++;
  if (!live.erase(p)) { printf("freed twice, or never allocated: %p\n", p); exit(3); }
  free(p);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) { if (s != STREAM) exit(4); call('S'); return hipSuccess; }
hipError_t hipSetDevice(int d) { if (d != 3) exit(4); call('D'); return hipSuccess; }
hipError_t hipGetLastError(void) { call('L'); return hipSuccess; }
}
struct Event { bool recorded = false; };
static std::set<void*> pinned;
static std::set<Event*> events;
static int refuse_host_next;
extern "C" {
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int flags) {
  if (flags != hipHostMallocDefault) exit(4);
  if (refuse_host_next > 0) { refuse_host_next--; call('h'); *p = nullptr; return hipErrorOutOfMemory; }
  call('H');
  *p = malloc(bytes);
  pinned.insert(*p);
  return hipSuccess;
}
hipError_t hipHostFree(void* p) {
  call('f');
  if (!pinned.erase(p)) { printf("pinned block freed twice, or never allocated: %p\n", p); exit(3); }
  free(p);
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  if (flags != hipEventDisableTiming) exit(4);
  call('E');
  Event* ev = new Event();
  events.insert(ev);
  *e = (hipEvent_t)ev;
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  if (s != STREAM || !events.count((Event*)e)) exit(4);
  call('R');
  ((Event*)e)->recorded = true;
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
  if (!events.count((Event*)e)) exit(4);
  if (!((Event*)e)->recorded) { printf("waited for an event that was never recorded\n"); exit(6); }
  call('W');
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  call('X');
  if (!events.erase((Event*)e)) { printf("event destroyed twice, or never created\n"); exit(3); }
  delete (Event*)e;
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
  if (s != STREAM || kind != hipMemcpyHostToDevice || !pinned.count((void*)src)) exit(4);
  call('C');
  memcpy(dst, src, bytes);
  return hipSuccess;
}
}

#define CHECK(c) do { if (!(c)) { printf("line %d: %s (calls so far: %s)\n", __LINE__, #c, calls.c_str()); exit(1); } } while (0)
// the calls since the last look, exactly
static bool made(const char* want) { const bool ok = calls == want; if (!ok) printf("calls were %s, expected %s\n", calls.c_str(), want); calls.clear(); return ok; }
static unsigned long long held() { return g_live_buffer_bytes.load(); }

struct Ctx { // what prv_ctx is to this header
  int device = 3;
  hipStream_t stream = STREAM;
  std::vector<Handle<Ctx>*> handles;
  BufferPool parked;
  PinnedStage pin;
  void end() { // prv_destroy's steps 2, 3 and 4
    detach_handles(this);
    parked.clear();
    pin.release();
  }
};
static hipError_t grow(Ctx& c, Buffer& b, size_t bytes, const char** call_out = nullptr) {
  const char* call = "";
  const hipError_t e = ensure(b, bytes, c.stream, c.parked, &call);
  if (call_out) *call_out = call;
  return e;
}

struct Child : Handle<Ctx> { // a trainer in small: two buffers, the second is parked when the child goes first
  using Handle<Ctx>::Handle;
  Buffer a, b;
  int retired = 0;
  void detach() override { a.reset(); b.reset(); }
  void retire() override { retired++; ctx->parked.park(std::move(b)); }
};

static void scope_exit_and_moves() {
  Ctx c;
  {
    Buffer b;
    CHECK(!b.p && b.bytes == 0);
    CHECK(grow(c, b, 64) == hipSuccess && b.p && b.bytes == 64 && held() == 64);
    Buffer empty;
    empty.reset(); // an empty buffer makes no call, reset or destroyed
  }
  CHECK(made("MF") && held() == 0);
  Buffer a, b;
  CHECK(grow(c, a, 8) == hipSuccess && grow(c, b, 16) == hipSuccess && made("MM"));
  void* pa = a.p;
  Buffer m(std::move(a)); // move-construct: the source lets go, nothing is freed
  CHECK(m.p == pa && m.bytes == 8 && !a.p && a.bytes == 0 && made("") && held() == 24);
  b = std::move(m); // move-assign over a live buffer: what b held is freed, once
  CHECK(b.p == pa && b.bytes == 8 && !m.p && made("F") && held() == 8);
  Buffer& self = b;
  b = std::move(self);
  CHECK(b.p == pa && b.bytes == 8 && made("") && held() == 8);
  b.reset();
  b.reset();
  CHECK(!b.p && made("F") && held() == 0);
}

static void growing() {
  Ctx c;
  Buffer b;
  CHECK(grow(c, b, 64) == hipSuccess && made("M"));
  void* first = b.p;
  CHECK(grow(c, b, 64) == hipSuccess && grow(c, b, 1) == hipSuccess && b.p == first && b.bytes == 64 && made("")); // grows only
  CHECK(grow(c, b, 65) == hipSuccess && b.bytes == 65 && live.count(first) == 0 && held() == 65);
  CHECK(made("SFM")); // the stream is synchronised, then the old block is freed (once), then the new one is allocated
}

static void out_of_memory() {
  Ctx c;
  Buffer parked1, parked2, b;
  CHECK(grow(c, parked1, 100) == hipSuccess && grow(c, parked2, 200) == hipSuccess);
  c.parked.park(std::move(parked1));
  c.parked.park(std::move(parked2));
  CHECK(c.parked.bytes == 300 && made("MM") && held() == 300);
  refuse_next = 1; // refused once: the pool is emptied behind a synchronise, the retry succeeds
  CHECK(grow(c, b, 50) == hipSuccess && b.p && b.bytes == 50);
  CHECK(made("mLSFFM") && c.parked.idle.empty() && c.parked.bytes == 0 && held() == 50);
  Buffer again;
  CHECK(grow(c, again, 10) == hipSuccess && made("M"));
  c.parked.park(std::move(again));
  refuse_next = 2; // the retry is refused too: b stays empty
  Buffer d;
  const char* call = nullptr;
  CHECK(grow(c, d, 70, &call) == hipErrorOutOfMemory && !d.p && d.bytes == 0 && std::string(call) == "e");
  CHECK(made("mLSFm") && held() == 50);
  refuse_next = 1; // nothing parked: no retry
  CHECK(grow(c, d, 70) == hipErrorOutOfMemory && !d.p && made("m"));
  refuse_next = 1; // a live buffer that cannot grow has lost its old block and holds nothing
  CHECK(grow(c, b, 51) == hipErrorOutOfMemory && !b.p && b.bytes == 0 && made("SFm") && held() == 0);
}

static void parking() {
  Ctx c;
  Buffer x, y, z;
  CHECK(grow(c, x, 10) == hipSuccess && grow(c, y, 20) == hipSuccess && grow(c, z, 10) == hipSuccess);
  void *px = x.p, *pz = z.p;
  c.parked.park(std::move(x));
  c.parked.park(std::move(y));
  c.parked.park(std::move(z));
  Buffer none;
  c.parked.park(std::move(none)); // an empty buffer is not parked
  CHECK(!x.p && !y.p && !z.p && c.parked.idle.size() == 3 && c.parked.bytes == 40 && made("MMM") && held() == 40);
  Buffer t;
  CHECK(!c.parked.take(t, 15) && !t.p);                                   // by exact size
  CHECK(c.parked.take(t, 10) && t.p == px && t.bytes == 10 && c.parked.bytes == 30); // the oldest of that size first
  Buffer u;
  CHECK(c.parked.take(u, 10) && u.p == pz && !c.parked.take(x, 10) && made("") && held() == 40);
  c.parked.clear();
  CHECK(made("F") && c.parked.bytes == 0);
  t.reset();
  u.reset();
  CHECK(made("FF") && held() == 0);
  // the count limit: the oldest goes when the 513th arrives
  void* oldest = nullptr;
  for (size_t i = 0; i < BufferPool::kMaxCount; i++) {
    Buffer b;
    CHECK(grow(c, b, 1000 + i) == hipSuccess);
    if (i == 0) oldest = b.p;
    c.parked.park(std::move(b));
  }
  CHECK(c.parked.idle.size() == BufferPool::kMaxCount && live.count(oldest) == 1);
  calls.clear();
  Buffer one_more;
  CHECK(grow(c, one_more, 7) == hipSuccess);
  c.parked.park(std::move(one_more));
  CHECK(made("MF") && c.parked.idle.size() == BufferPool::kMaxCount && live.count(oldest) == 0 && !c.parked.take(t, 1000) && c.parked.take(t, 1001));
  t.reset();
  c.parked.clear();
  calls.clear();
  CHECK(held() == 0 && live.empty());
  // the byte limit: 16 GiB in all, oldest first; a block larger than that is freed, not parked
  const size_t GiB = (size_t)1 << 30;
  Buffer g10, g5, g2, g17;
  CHECK(grow(c, g10, 10 * GiB) == hipSuccess && grow(c, g5, 5 * GiB) == hipSuccess && grow(c, g2, 2 * GiB) == hipSuccess && grow(c, g17, 17 * GiB) == hipSuccess);
  c.parked.park(std::move(g10));
  c.parked.park(std::move(g5));
  CHECK(made("MMMM") && c.parked.bytes == 15 * GiB);
  c.parked.park(std::move(g2)); // 17 GiB would be parked: the 10 GiB block, the oldest, goes
  CHECK(made("F") && c.parked.bytes == 7 * GiB && c.parked.idle.size() == 2 && !g2.p);
  c.parked.park(std::move(g17));
  CHECK(made("F") && c.parked.bytes == 7 * GiB && c.parked.idle.size() == 2 && !g17.p && held() == 7 * GiB);
  c.parked.clear();
  CHECK(made("FF") && held() == 0);
}

static void child_before_context() {
  Ctx c;
  Child* h = new Child(&c);
  CHECK(c.handles.size() == 1 && c.handles[0] == h && h->ctx == &c);
  CHECK(grow(c, h->a, 30) == hipSuccess && grow(c, h->b, 40) == hipSuccess && made("MM"));
  Child* other = new Child(&c);
  destroy_handle(h); // device current, context stream drained, the child's last words, then its destructor
  CHECK(made("DSF") && c.handles.size() == 1 && c.handles[0] == other && c.parked.bytes == 40 && held() == 40);
  destroy_handle(other);
  destroy_handle((Child*)nullptr);
  CHECK(made("DS") && c.handles.empty());
  c.end();
  CHECK(made("F") && held() == 0);
}

static void context_before_child() {
  Ctx* c = new Ctx();
  Child* h = new Child(c);
  CHECK(grow(*c, h->a, 30) == hipSuccess && grow(*c, h->b, 40) == hipSuccess && made("MM"));
  c->end();
  CHECK(made("FF") && h->ctx == nullptr && !h->a.p && !h->b.p && c->handles.empty() && held() == 0);
  delete c;
  frozen = true; // the device may have been reset by now: an inert handle makes no runtime call and frees nothing twice
  destroy_handle(h);
  frozen = false;
  CHECK(made(""));
}

static int create(Ctx& c, bool fail, Child** out) { // the shape of every prv_*_create
  std::unique_ptr<Child> h(new Child(&c));
  if (grow(c, h->a, 8) != hipSuccess) return -1;
  if (fail) return -23; // between an allocation and handing the handle out
  if (grow(c, h->b, 8) != hipSuccess) return -2;
  *out = h.release();
  return 0;
}

static void early_return() {
  Ctx c;
  Child* h = nullptr;
  CHECK(create(c, true, &h) == -23 && !h && made("MF") && c.handles.empty() && held() == 0);
  refuse_next = 1;
  CHECK(create(c, false, &h) == -1 && !h && made("m") && c.handles.empty());
  CHECK(create(c, false, &h) == 0 && h && made("MM") && c.handles.size() == 1 && held() == 16);
  c.end();
  destroy_handle(h);
  CHECK(made("FF") && held() == 0);
}

static hipError_t acquire(PinnedStage& s, size_t bytes, void** p, const char** call_out = nullptr) {
  const char* call = "";
  const hipError_t e = s.acquire(bytes, p, &call);
  if (call_out) *call_out = call;
  return e;
}
static hipError_t send(PinnedStage& s, void* dst, size_t bytes) {
  const char* call = "";
  return s.send(dst, bytes, STREAM, &call);
}

static void pinned_stage() {
  static char dev[16384];
  Ctx* c = new Ctx();
  PinnedStage& s = c->pin;
  void *p = nullptr, *q = nullptr;
  CHECK(acquire(s, 100, &p) == hipSuccess && p && s.cap == 8192 && made("HE")); // first use: the block (8192 at the least), the event, no wait
  memset(p, 1, 8192);
  CHECK(acquire(s, 8192, &q) == hipSuccess && q == p && made("")); // the caller returned early, nothing was sent: nothing to wait for
  CHECK(send(s, dev, 100) == hipSuccess && dev[99] == 1 && dev[100] == 0 && made("CR"));
  CHECK(acquire(s, 8192, &q) == hipSuccess && q == p && made("W")); // after a send: the wait, no allocation
  CHECK(acquire(s, 1, &q) == hipSuccess && q == p && made(""));      // ... once
  CHECK(send(s, dev, 8192) == hipSuccess && made("CR"));
  CHECK(acquire(s, 8193, &p) == hipSuccess && s.cap == 8193 && made("WfH")); // growth in flight: wait, then free, then allocate
  memset(p, 2, 8193);
  CHECK(acquire(s, 9000, &p) == hipSuccess && s.cap == 9000 && made("fH")); // growth with nothing in flight
  CHECK(send(s, dev, 9000) == hipSuccess && made("CR"));
  refuse_host_next = 1; // refused: the old block went (once), the stage is empty, the event stays
  const char* call = nullptr;
  CHECK(acquire(s, 10000, &q, &call) == hipErrorOutOfMemory && !s.p && s.cap == 0 && s.ev && made("Wfh"));
  CHECK(std::string(call) == "hipHostMalloc(&c->pin, std::max<size_t>(up_bytes, 8192), hipHostMallocDefault)");
  CHECK(acquire(s, 100, &p) == hipSuccess && p && s.cap == 8192 && made("H")); // ... and usable again, with nothing to wait for
  CHECK(send(s, dev, 100) == hipSuccess && made("CR"));
  {
    PinnedStage m(std::move(s)); // move-construct: the source lets go of block, event and the pending wait; no call
    CHECK(m.p == p && m.cap == 8192 && m.ev && !s.p && !s.cap && !s.ev && made(""));
    CHECK(acquire(m, 10, &q) == hipSuccess && q == p && made("W"));
    PinnedStage other;
    CHECK(acquire(other, 10, &q) == hipSuccess && q != p && made("HE"));
    other = std::move(m); // move-assign over a live stage: what it held goes, once
    CHECK(other.p == p && !m.p && !m.ev && made("fX"));
    PinnedStage& self = other;
    other = std::move(self);
    CHECK(other.p == p && made(""));
    s = std::move(other);
    CHECK(s.p == p && made(""));
  } // (m and other are empty: no call)
  CHECK(made(""));
  {
    PinnedStage local, empty;
    CHECK(acquire(local, 10, &q) == hipSuccess && made("HE"));
    empty.release();
  }
  CHECK(made("fX") && pinned.size() == 1 && events.size() == 1); // destruction: one free, one event destroyed
  CHECK(send(s, dev, 10) == hipSuccess && made("CR"));
  c->end(); // (prv_destroy has drained the stream: no wait)
  CHECK(made("fX") && pinned.empty() && events.empty());
  frozen = true; // no runtime call follows the context's end
  delete c;
  frozen = false;
  CHECK(made(""));
}

int main() { // (after each case: what its locals freed when they left their scope)
  scope_exit_and_moves();
  CHECK(made(""));
  growing();
  CHECK(made("F"));
  out_of_memory();
  CHECK(made(""));
  parking();
  CHECK(made(""));
  child_before_context();
  context_before_child();
  early_return();
  pinned_stage();
  CHECK(made("") && pinned.empty() && events.empty());
  CHECK(made("") && live.empty() && n_malloc == n_free && held() == 0);
  printf("ok %d\n", n_malloc);
  return 0;
}
"""


def test_buffers_and_handles_free_what_they_hold_exactly_once(tmp_path):
    src, exe = tmp_path / "buffers.cpp", tmp_path / "buffers"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "nerf_prv_amd", "csrc"), "-isystem", os.path.join(ROCM, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], text=True, capture_output=True, timeout=60)
    assert out.returncode == 0 and out.stdout == "ok 536\n", out.stdout + out.stderr
