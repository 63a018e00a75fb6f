"""csrc/seg_args.h on its own: the buffer table's checker and the shared size rule, compiled into a small host program
(with the address and undefined-behaviour sanitizers where the compiler has them) that needs neither the library nor a
device.  What the eight entry points do with it is in their own CPU tests, through tests/seg_args_cases.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <stdio.h>
#include "seg_args.h"
using namespace dfw;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

int main() {
  alignas(16) static unsigned char m[256];
  {  // touching end to start is fine, one shared byte is not; extents are half-open
    const seg_buf t[] = {seg_in(m, 16), seg_out(m + 16, 16, 4), seg_out(m + 32, 8, 8), seg_out(m + 40, 24, 4)};
    CHECK(seg_check_buffers(t) == 0);
    const seg_buf u[] = {seg_in(m, 17), seg_out(m + 16, 16, 4)};
    CHECK(seg_check_buffers(u) == DFW_EINVAL);
    const seg_buf v[] = {seg_out(m + 16, 16, 4), seg_out(m + 31, 8)};
    CHECK(seg_check_buffers(v) == DFW_EINVAL);
    const seg_buf w[] = {seg_out(m + 32, 8), seg_in(m, 64)};          // an input around an output
    CHECK(seg_check_buffers(w) == DFW_EINVAL);
  }
  {  // two inputs may alias; a null pointer or an empty extent is absent, wherever it points and whatever it asks for
    const seg_buf t[] = {seg_in(m, 64), seg_in(m, 64), seg_in(m + 8, 8, 4), seg_out(m + 64, 4, 4)};
    CHECK(seg_check_buffers(t) == 0);
    const seg_buf u[] = {seg_in(m, 64), seg_out(nullptr, 64, 8), seg_out(m + 3, 0, 8), seg_out(m + 64, 4, 4)};
    CHECK(seg_check_buffers(u) == 0);
  }
  {  // alignment: only after overlap, only for present buffers, 0 and 1 mean none
    const seg_buf t[] = {seg_in(m + 1, 7), seg_out(m + 9, 3, 0), seg_out(m + 16, 16, 16)};
    CHECK(seg_check_buffers(t) == 0);
    const seg_buf u[] = {seg_in(m, 8), seg_out(m + 18, 4, 4)};
    CHECK(seg_check_buffers(u) == DFW_ESHAPE);
    const seg_buf v[] = {seg_in(m + 2, 8, 4), seg_out(m + 16, 4, 4)};
    CHECK(seg_check_buffers(v) == DFW_ESHAPE);
    const seg_buf w[] = {seg_in(m, 8), seg_out(m + 6, 4, 4)};          // on the input AND off its alignment
    CHECK(seg_check_buffers(w) == DFW_EINVAL);
    const seg_buf x[] = {seg_in(m, 8), seg_out(m + 24, 16, 16)};
    CHECK(seg_check_buffers(x) == DFW_ESHAPE);
  }
  CHECK(seg_overlap(m, 4, m + 3, 4) && !seg_overlap(m, 4, m + 4, 4) && !seg_overlap(m, 0, m, 4) && !seg_overlap(nullptr, 4, m, 4));
  // the size rule: DFW_EINVAL before DFW_ERANGE
  CHECK(seg_map_size_error(1, 1, 1) == 0 && seg_map_size_error(65535, 32768, 32768) == 0);
  CHECK(seg_map_size_error(65535, 65535, 16384) == 0);
  CHECK(seg_map_size_error(0, 5, 5) == DFW_EINVAL && seg_map_size_error(1, -1, 5) == DFW_EINVAL);
  CHECK(seg_map_size_error(1, 5, 0) == DFW_EINVAL && seg_map_size_error(0, 65536, 5) == DFW_EINVAL);
  CHECK(seg_map_size_error(65536, 1, 1) == DFW_ERANGE && seg_map_size_error(1, 65536, 1) == DFW_ERANGE);
  CHECK(seg_map_size_error(1, 1, 65536) == DFW_ERANGE && seg_map_size_error(1, 65535, 32768) == DFW_ERANGE);
  CHECK(seg_map_size_error(1, 32768, 32769) == DFW_ERANGE);
  printf("%d\n", fails);
  return fails != 0;
}
'''


def test_checker_and_size_rule_in_a_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "seg_args_check.cpp", tmp_path / "seg_args_check"
    src.write_text(PROGRAM)
    base = [cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-I", os.path.join(ROOT, "diffews_amd", "csrc"), str(src), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:                                              # a compiler without the sanitizers' runtime
        subprocess.run(base, check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0", r.stdout + r.stderr


def test_the_header_is_host_only_and_the_stages_use_it():
    csrc = os.path.join(ROOT, "diffews_amd", "csrc")
    text = open(os.path.join(csrc, "seg_args.h")).read()
    assert "__global__" not in text and "__device__" not in text and "hip_runtime" not in text and "common.h" not in text
    stages = ("seg_components", "seg_holes", "seg_rle", "seg_contours", "seg_match", "seg_scores", "seg_boundary")
    for name in stages:
        src = open(os.path.join(csrc, name + ".hip")).read()
        assert '#include "seg_args.h"' in src and "seg_check_buffers(" in src, name
    assert open(os.path.join(csrc, "seg_boundary.hip")).read().count("seg_check_buffers(") == 2      # and its counts
    # one copy of each helper
    every = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)))
    assert every.count("bool seg_overlap(") == 1 and "sh_overlap" not in every
    assert every.count("> 65535 || W > 65535 || H * W > (1ll << 30)") == 1
