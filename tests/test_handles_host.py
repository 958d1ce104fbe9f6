"""The planner shell's owners of C-ABI objects (nerf_prv_amd/host/prv_handles.hpp) against a counting stub of the calls
they make: whatever is acquired is released exactly once -- at scope exit, across moves, and on an early return between two
acquisitions.  Host code only: a stand-alone program built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "prv_handles.hpp"
#include <cstdio>
#include <cstdlib>
#include <set>
using namespace prvhost;

// ---- the counting stub: every object is a heap block, so a double release or a leak is also the sanitizer's finding
static int n_malloc, n_free, n_camset, n_camset_destroy, n_index, n_index_destroy, n_mesh, n_mesh_destroy, n_train, n_train_destroy;
static std::set<void*> live;
static void* make(int& counter) { counter++; void* p = malloc(8); live.insert(p); return p; }
static void drop(void* p, int& counter) {
  counter++;
  if (!live.erase(p)) { printf("released twice, or never acquired: %p\n", p); exit(3); }
  free(p);
}
static prv_ctx* const CTX = (prv_ctx*)0x10;
extern "C" {
int prv_malloc(prv_ctx* ctx, void** out, size_t bytes) {
  if (ctx != CTX) exit(4);
  if (bytes == 0) { *out = nullptr; return PRV_E_INVALID; }
  *out = make(n_malloc);
  return PRV_OK;
}
int prv_free(prv_ctx* ctx, void* p) { if (ctx != CTX) exit(4); drop(p, n_free); return PRV_OK; }
int prv_cameras_from_json(prv_ctx*, const char* path, prv_camset** out) {
  if (!path[0]) { *out = nullptr; return PRV_E_IO; }
  *out = (prv_camset*)make(n_camset);
  return PRV_OK;
}
void prv_camset_destroy(prv_camset* c) { drop(c, n_camset_destroy); }
int prv_nn_index_create(prv_ctx*, const float*, uint64_t, const prv_nn_opts*, prv_nn_index** out) { *out = (prv_nn_index*)make(n_index); return PRV_OK; }
void prv_nn_index_destroy(prv_nn_index* i) { drop(i, n_index_destroy); }
int prv_marching_cubes(prv_ctx*, int, const prv_mesh_opts*, prv_mesh** out) { *out = (prv_mesh*)make(n_mesh); return PRV_OK; }
void prv_mesh_destroy(prv_mesh* m) { drop(m, n_mesh_destroy); }
int prv_train_create(prv_ctx*, int, const prv_camset*, const uint8_t*, int, int, const prv_train_opts*, prv_trainer** out) {
  *out = (prv_trainer*)make(n_train);
  return PRV_OK;
}
void prv_train_destroy(prv_trainer* t) { drop(t, n_train_destroy); }
}

#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static void acquire_then_scope_exit() {
  {
    DeviceArray<float> a;
    CHECK(!a && a.get() == nullptr);
    CHECK(a.alloc(CTX, 64) == PRV_OK && a && a.get());
    CamsetPtr cams;
    CHECK(prv_cameras_from_json(CTX, "x.json", out_arg(cams)) == PRV_OK); // (the handle is filled when the statement ends)
    CHECK(cams);
    NnIndexPtr index;
    CHECK(prv_nn_index_create(CTX, a.get(), 1, nullptr, out_arg(index)) == PRV_OK);
    CHECK(index);
    MeshPtr mesh;
    CHECK(prv_marching_cubes(CTX, 0, nullptr, out_arg(mesh)) == PRV_OK);
    CHECK(mesh);
    std::vector<TrainerPtr> trs;
    for (int k = 0; k < 3; k++) {
      TrainerPtr t;
      CHECK(prv_train_create(CTX, k, cams.get(), nullptr, 1, 1, nullptr, out_arg(t)) == PRV_OK);
      CHECK(t);
      trs.push_back(std::move(t));
    }
    CHECK(raw_trainers(trs).size() == 3 && raw_trainers(trs)[2] == trs[2].get());
    trs.clear(); // the shell's explicit order: trainers first
    CHECK(n_train_destroy == 3 && n_camset_destroy == 0 && n_free == 0);
  }
  CHECK(n_free == 1 && n_camset_destroy == 1 && n_index_destroy == 1 && n_mesh_destroy == 1);
  {
    DeviceArray<uint8_t> failed; // a refused allocation holds nothing and releases nothing
    CHECK(failed.alloc(CTX, 0) != PRV_OK && !failed);
    CamsetPtr none;
    CHECK(prv_cameras_from_json(CTX, "", out_arg(none)) != PRV_OK);
    CHECK(!none);
    DeviceArray<uint8_t> again; // a second allocation into a live handle releases the first
    CHECK(again.alloc(CTX, 8) == PRV_OK && again.alloc(CTX, 16) == PRV_OK);
    CHECK(n_malloc == 3 && n_free == 2);
    again.reset();
    again.reset();
    CHECK(n_free == 3);
  }
  CHECK(n_free == 3 && n_camset == 1);
}

static void moves() {
  DeviceArray<float> a, b;
  CHECK(a.alloc(CTX, 8) == PRV_OK && b.alloc(CTX, 8) == PRV_OK);
  float* pa = a.get();
  const int freed = n_free;
  DeviceArray<float> c(std::move(a)); // move-construct: the source lets go, nothing is released
  CHECK(c.get() == pa && !a && n_free == freed);
  b = std::move(c); // move-assign over a live handle: what b held is released, once
  CHECK(b.get() == pa && !c && n_free == freed + 1);
  DeviceArray<float>& self = b;
  b = std::move(self);
  CHECK(b.get() == pa && n_free == freed + 1);
  CamsetPtr x, y;
  CHECK(prv_cameras_from_json(CTX, "x", out_arg(x)) == PRV_OK);
  CHECK(prv_cameras_from_json(CTX, "y", out_arg(y)) == PRV_OK);
  const int destroyed = n_camset_destroy;
  y = std::move(x);
  CHECK(!x && y && n_camset_destroy == destroyed + 1);
  CHECK(prv_cameras_from_json(CTX, "z", out_arg(y)) == PRV_OK); // refilled through out_arg: what it held goes
  CHECK(y && n_camset_destroy == destroyed + 2);
}

static int early_return(bool fail) {
  CamsetPtr cams;
  if (prv_cameras_from_json(CTX, "x", out_arg(cams)) != PRV_OK) return -1;
  DeviceArray<float> first;
  if (first.alloc(CTX, 8) != PRV_OK) return -2;
  if (fail) return -23; // between two acquisitions
  DeviceArray<float> second;
  if (second.alloc(CTX, 8) != PRV_OK) return -3;
  return 0;
}

int main() {
  acquire_then_scope_exit();
  moves();
  CHECK(early_return(true) == -23 && early_return(false) == 0);
  CHECK(live.empty());
  CHECK(n_malloc == n_free && n_camset == n_camset_destroy && n_index == n_index_destroy && n_mesh == n_mesh_destroy && n_train == n_train_destroy);
  CHECK(n_malloc == 8 && n_camset == 6 && n_index == 1 && n_mesh == 1 && n_train == 3);
  printf("ok\n");
  return 0;
}
"""


def test_handles_release_what_they_acquire_exactly_once(tmp_path):
    src, exe = tmp_path / "handles.cpp", tmp_path / "handles"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "nerf_prv_amd", "host"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], text=True, capture_output=True, timeout=60)
    assert out.returncode == 0 and out.stdout == "ok\n", out.stdout + out.stderr
