"""csrc/dispatch.h on the host: one_of picks the listed constant, else the default, exactly once.

A stand-alone C++17 program (its own main, dispatch.h its only project include) built with
address and undefined-behaviour sanitizers and run as a child process. No GPU, nothing loaded
into Python.
"""
import pathlib
import subprocess

import pytest

CXX = pathlib.Path("/opt/rocm/llvm/bin/clang++")
CSRC = pathlib.Path(__file__).resolve().parents[1] / "lesion_gnn_amd" / "csrc"

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "dispatch.h"

#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                            \
    }                                                          \
  } while (0)

template <int P, bool V, int NC>
struct Kernel {
  static int id() { return P * 1000 + (V ? 100 : 0) + NC; }
};
template <int N>
int as_template_arg() { return N; }

int main() {
  // a listed value reaches f as that constant, an unlisted one as the default; f runs once
  const int asked[] = {0, 1, 2, 3, 4, 5, 8, 16, 17, 18, -1};
  for (int v : asked) {
    int calls = 0, got = -99;
    one_of<0, 2, 4, 8, 17>(v, [&](auto NC) {
      ++calls;
      got = NC;
      static_assert(std::is_same<typename decltype(NC)::value_type, int>::value, "int constant");
      CHECK(as_template_arg<NC>() == NC);  // usable as a template argument
    });
    const bool listed = v == 2 || v == 4 || v == 8 || v == 17;
    CHECK(calls == 1);
    CHECK(got == (listed ? v : 0));
  }
  // the default is its own arm even when a listed value is numerically equal in another type
  for (int v : {0, 1, 2}) {
    int calls = 0, as_bool = 0, as_int = 0;
    one_of<false, 0, 1>(v, [&](auto X) {
      ++calls;
      if constexpr (std::is_same<typename decltype(X)::value_type, bool>::value) ++as_bool;
      else ++as_int;
      CHECK((int)X == (v == 1 ? 1 : 0));
    });
    CHECK(calls == 1);
    CHECK(as_int == (v <= 1 ? 1 : 0) && as_bool == (v == 2 ? 1 : 0));
  }
  // the default listed again: still one call
  for (int v : {1, 3, 7}) {
    int calls = 0, got = 0;
    one_of<1, 1, 3>(v, [&](auto P) { ++calls; got = P; });
    CHECK(calls == 1 && got == (v == 3 ? 3 : 1));
  }
  // bool: default false, listed true
  for (bool v : {false, true}) {
    int calls = 0;
    bool got = !v;
    one_of<false, true>(v, [&](auto V) { ++calls; got = V; });
    CHECK(calls == 1 && got == v);
  }
  // no list at all: the default
  {
    int calls = 0;
    one_of<7>(3, [&](auto D) { ++calls; CHECK(D == 7); });
    CHECK(calls == 1);
  }
  // a three-deep nest visits exactly one leaf, with the three constants as template arguments
  for (int planes : {1, 3, 2})
    for (bool v : {false, true})
      for (int nck : {0, 2, 3, 4, 8, 17, 40}) {
        int leaves = 0, id = -1;
        one_of<1, 3>(planes, [&](auto P) {
          one_of<false, true>(v, [&](auto V) {
            one_of<0, 2, 4, 8, 17>(nck, [&](auto NC) {
              ++leaves;
              id = Kernel<P, V, NC>::id();
            });
          });
        });
        const int nc = (nck == 2 || nck == 4 || nck == 8 || nck == 17) ? nck : 0;
        CHECK(leaves == 1);
        CHECK(id == (planes == 3 ? 3 : 1) * 1000 + (v ? 100 : 0) + nc);
      }
  // a dependent argument derived inside the lambda
  for (int nl : {1, 2, 3, 4, 9}) {
    int calls = 0;
    one_of<1, 2, 3, 4>(nl, [&](auto NL) {
      constexpr bool XIN = NL == 4;
      ++calls;
      CHECK(XIN == (nl == 4));
    });
    CHECK(calls == 1);
  }
  std::puts("dispatch ok");
  return 0;
}
"""


@pytest.mark.skipif(not CXX.exists(), reason="no clang++ to build the host program with")
def test_one_of_host_sanitized(tmp_path):
    src, exe = tmp_path / "dispatch_host.cpp", tmp_path / "dispatch_host"
    src.write_text(PROGRAM)
    build = subprocess.run(
        [str(CXX), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", f"-I{CSRC}", str(src), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "dispatch ok"
