// prv_handles.hpp -- move-only owners of what the planner shell allocates through include/prv.h: device memory, camera
// sets, the nearest-neighbour index, meshes, coverage handles and trainers.  A handle releases what it holds when it leaves its scope, so an
// early return between two acquisitions leaks nothing.  prv_planner-private (the functions named here are libprv_hip's):
// included by main.cpp's side only, never by a file of libprv_host.so.
#pragma once
#include <cstddef>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/prv.h"

namespace prvhost {

struct CamsetDelete {
  void operator()(prv_camset* c) const { prv_camset_destroy(c); }
};
struct NnIndexDelete {
  void operator()(prv_nn_index* i) const { prv_nn_index_destroy(i); }
};
struct MeshDelete {
  void operator()(prv_mesh* m) const { prv_mesh_destroy(m); }
};
struct CoverageDelete {
  void operator()(prv_coverage* c) const { prv_coverage_destroy(c); }
};
struct TrainerDelete {
  void operator()(prv_trainer* t) const { prv_train_destroy(t); }
};
using CamsetPtr = std::unique_ptr<prv_camset, CamsetDelete>;
using NnIndexPtr = std::unique_ptr<prv_nn_index, NnIndexDelete>;
using MeshPtr = std::unique_ptr<prv_mesh, MeshDelete>;
using CoveragePtr = std::unique_ptr<prv_coverage, CoverageDelete>;
using TrainerPtr = std::unique_ptr<prv_trainer, TrainerDelete>;

// the C ABI hands objects out through an out-parameter: `prv_cameras_from_json(ctx, path, out_arg(cams))` fills the handle
// (and releases what it held) when the STATEMENT that makes the call ends -- look at the handle in the next one, not in
// the same expression.  The shape of C++23's std::out_ptr.
template <class Ptr> class OutArg {
public:
  explicit OutArg(Ptr& p) : owner(p) {}
  OutArg(const OutArg&) = delete;
  OutArg& operator=(const OutArg&) = delete;
  ~OutArg() { owner.reset(raw); }
  operator typename Ptr::pointer*() { return &raw; }

private:
  Ptr& owner;
  typename Ptr::pointer raw = nullptr;
};
template <class Ptr> OutArg<Ptr> out_arg(Ptr& p) { return OutArg<Ptr>(p); }

// what prv_train_steps_multi and friends take: the trainers of a list, still owned by the list
inline std::vector<prv_trainer*> raw_trainers(const std::vector<TrainerPtr>& trs) {
  std::vector<prv_trainer*> raw;
  for (const TrainerPtr& t : trs) raw.push_back(t.get());
  return raw;
}

// device memory of prv_malloc: prv_free needs the context, so it travels with the pointer
template <class T> class DeviceArray {
public:
  DeviceArray() = default;
  DeviceArray(const DeviceArray&) = delete;
  DeviceArray& operator=(const DeviceArray&) = delete;
  DeviceArray(DeviceArray&& o) noexcept : ctx(o.ctx), ptr(o.ptr) { o.ptr = nullptr; }
  DeviceArray& operator=(DeviceArray&& o) noexcept {
    if (this != &o) {
      reset();
      ctx = o.ctx;
      ptr = o.ptr;
      o.ptr = nullptr;
    }
    return *this;
  }
  ~DeviceArray() { reset(); }

  // `bytes` of device memory (what was held is released first); prv_malloc's return code
  int alloc(prv_ctx* c, size_t bytes) {
    reset();
    ctx = c;
    void* p = nullptr;
    const int rc = prv_malloc(ctx, &p, bytes);
    ptr = rc == PRV_OK ? static_cast<T*>(p) : nullptr;
    return rc;
  }
  void reset() {
    if (ptr) prv_free(ctx, ptr);
    ptr = nullptr;
  }
  T* get() const { return ptr; }
  explicit operator bool() const { return ptr != nullptr; }

private:
  prv_ctx* ctx = nullptr;
  T* ptr = nullptr;
};

} // namespace prvhost
