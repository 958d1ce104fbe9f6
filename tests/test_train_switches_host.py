"""The trainer's PRV_TRAIN_* environment switches (nerf_prv_amd/csrc/prv_train_switches.hpp) parse as they did when every
switch was read where it was used.  Host code only: a stand-alone program built with the address and undefined-behaviour
sanitizers sets and unsets the variables and checks the parsed struct.

The rules, as the code that read each switch in place stated them (e = getenv(NAME)):
  PRV_TRAIN_GRAPH         if (e) use_graph = atoi(e) != 0;                    else true
  PRV_TRAIN_FAST_FWD      if (e) fast_forward = atoi(e) != 0;                 else true
  PRV_TRAIN_REG_CHAIN     if (e) reg_chain = atoi(e) != 0;                    else true
  PRV_TRAIN_KEEP_ACT      if (e) keep_act = keep_act && atoi(e) != 0;         else true (and only on the fast path: the trainer's part)
  PRV_TRAIN_OWN_QUEUE     own_queue = !(e && atoi(e) == 0)                    -- the same rule: on unless atoi reads 0
  PRV_TRAIN_TILE_SKIP     live_off = e && atoi(e) == 0                        -- the same rule
  PRV_TRAIN_LIST_AHEAD    off = e && atoi(e) == 0                             -- the same rule
  PRV_TRAIN_PATCH_JITTER  if (e) patch_ray_jitter = !strcmp(e, "ray");        else false
  PRV_TRAIN_ACT_CAP       if (e) cap = max(32, atoi(e));                      else sized from the sample budget (0 here)
  PRV_TRAIN_BWD_BLOCKS    over = e ? atoi(e) : 0; used when over > 0          (the clamp to two blocks per CU is the trainer's part)
  PRV_TRAIN_FWD_BLOCKS    fwd_over = e ? atoi(e) : 0; used when fwd_over > 0
  PRV_TRAIN_TIMING        timing = e != nullptr
so "0", the empty string and junk such as "abc" all switch an on/off switch OFF (atoi reads 0), and "1" or "7" switch it on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "prv_train_switches.hpp"
#include <cstdio>
#include <string>
using prv::TrainSwitches;

#define CHECK(c) do { if (!(c)) { printf("line %d: %s (with %s)\n", __LINE__, #c, what.c_str()); exit(1); } } while (0)
static std::string what = "nothing set";
static int n_checks;

static const char* const ALL[] = {"PRV_TRAIN_GRAPH", "PRV_TRAIN_FAST_FWD", "PRV_TRAIN_REG_CHAIN", "PRV_TRAIN_KEEP_ACT", "PRV_TRAIN_OWN_QUEUE",
                                  "PRV_TRAIN_TILE_SKIP", "PRV_TRAIN_LIST_AHEAD", "PRV_TRAIN_PATCH_JITTER", "PRV_TRAIN_ACT_CAP",
                                  "PRV_TRAIN_BWD_BLOCKS", "PRV_TRAIN_FWD_BLOCKS", "PRV_TRAIN_TIMING"};
struct OnOff { const char* name; bool TrainSwitches::*field; };
static const OnOff ON_OFF[] = {{"PRV_TRAIN_GRAPH", &TrainSwitches::use_graph}, {"PRV_TRAIN_FAST_FWD", &TrainSwitches::fast_forward},
                               {"PRV_TRAIN_REG_CHAIN", &TrainSwitches::reg_chain}, {"PRV_TRAIN_KEEP_ACT", &TrainSwitches::keep_act},
                               {"PRV_TRAIN_OWN_QUEUE", &TrainSwitches::own_queue}, {"PRV_TRAIN_TILE_SKIP", &TrainSwitches::tile_skip},
                               {"PRV_TRAIN_LIST_AHEAD", &TrainSwitches::list_ahead}};

// every field but the named one (NULL: every field) holds its default
static void others_default(const TrainSwitches& s, const char* but) {
  const std::string b = but ? but : "";
  for (const OnOff& o : ON_OFF)
    if (b != o.name) CHECK(s.*o.field == true);
  if (b != "PRV_TRAIN_PATCH_JITTER") CHECK(s.patch_ray_jitter == false);
  if (b != "PRV_TRAIN_ACT_CAP") CHECK(s.act_cap == 0);
  if (b != "PRV_TRAIN_BWD_BLOCKS") CHECK(s.bwd_blocks == 0);
  if (b != "PRV_TRAIN_FWD_BLOCKS") CHECK(s.fwd_blocks == 0);
  if (b != "PRV_TRAIN_TIMING") CHECK(s.timing == false);
  n_checks++;
}

// one variable set, the other eleven unset
static TrainSwitches with(const char* name, const char* value) {
  for (const char* n : ALL) unsetenv(n);
  setenv(name, value, 1);
  what = std::string(name) + "='" + value + "'";
  const TrainSwitches s = prv::train_switches_from_env();
  others_default(s, name);
  return s;
}

int main() {
  for (const char* n : ALL) unsetenv(n);
  others_default(prv::train_switches_from_env(), nullptr);
  for (const OnOff& o : ON_OFF) {
    CHECK(with(o.name, "0").*o.field == false);
    CHECK(with(o.name, "1").*o.field == true);
    CHECK(with(o.name, "7").*o.field == true);
    CHECK(with(o.name, "").*o.field == false);
    CHECK(with(o.name, "abc").*o.field == false);
    CHECK(with(o.name, "0x1").*o.field == false); // atoi stops at the x
  }
  CHECK(with("PRV_TRAIN_PATCH_JITTER", "ray").patch_ray_jitter == true);
  for (const char* v : {"", "1", "Ray", "rays", " ray", "pixel"}) CHECK(with("PRV_TRAIN_PATCH_JITTER", v).patch_ray_jitter == false);
  CHECK(with("PRV_TRAIN_ACT_CAP", "1").act_cap == 32);
  CHECK(with("PRV_TRAIN_ACT_CAP", "").act_cap == 32);
  CHECK(with("PRV_TRAIN_ACT_CAP", "abc").act_cap == 32);
  CHECK(with("PRV_TRAIN_ACT_CAP", "-5").act_cap == 32);
  CHECK(with("PRV_TRAIN_ACT_CAP", "32").act_cap == 32);
  CHECK(with("PRV_TRAIN_ACT_CAP", "33").act_cap == 33);
  CHECK(with("PRV_TRAIN_ACT_CAP", "256").act_cap == 256);
  CHECK(with("PRV_TRAIN_BWD_BLOCKS", "0").bwd_blocks == 0);
  CHECK(with("PRV_TRAIN_BWD_BLOCKS", "-3").bwd_blocks == 0);
  CHECK(with("PRV_TRAIN_BWD_BLOCKS", "64").bwd_blocks == 64);
  CHECK(with("PRV_TRAIN_BWD_BLOCKS", "abc").bwd_blocks == 0);
  CHECK(with("PRV_TRAIN_BWD_BLOCKS", "100000").bwd_blocks == 100000); // (the trainer clamps it to two blocks per CU)
  CHECK(with("PRV_TRAIN_FWD_BLOCKS", "0").fwd_blocks == 0);
  CHECK(with("PRV_TRAIN_FWD_BLOCKS", "-3").fwd_blocks == 0);
  CHECK(with("PRV_TRAIN_FWD_BLOCKS", "64").fwd_blocks == 64);
  CHECK(with("PRV_TRAIN_TIMING", "").timing == true);
  CHECK(with("PRV_TRAIN_TIMING", "0").timing == true);
  CHECK(with("PRV_TRAIN_TIMING", "1").timing == true);
  // read when asked, not once per process: the same variable, changed between two reads
  CHECK(with("PRV_TRAIN_TILE_SKIP", "0").tile_skip == false && with("PRV_TRAIN_TILE_SKIP", "1").tile_skip == true);
  // all twelve at once
  for (const char* n : ALL) setenv(n, "0", 1);
  setenv("PRV_TRAIN_PATCH_JITTER", "ray", 1);
  setenv("PRV_TRAIN_ACT_CAP", "4096", 1);
  setenv("PRV_TRAIN_BWD_BLOCKS", "12", 1);
  setenv("PRV_TRAIN_FWD_BLOCKS", "34", 1);
  what = "all twelve set";
  const TrainSwitches s = prv::train_switches_from_env();
  for (const OnOff& o : ON_OFF) CHECK(s.*o.field == false);
  CHECK(s.patch_ray_jitter && s.act_cap == 4096 && s.bwd_blocks == 12 && s.fwd_blocks == 34 && s.timing);
  printf("ok %d\n", n_checks);
  return 0;
}
"""


def test_the_trainer_switches_parse_by_the_rules_of_the_code_they_replace(tmp_path):
    src, exe = tmp_path / "switches.cpp", tmp_path / "switches"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "nerf_prv_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], text=True, capture_output=True, timeout=60)
    assert out.returncode == 0 and out.stdout == "ok 70\n", out.stdout + out.stderr
