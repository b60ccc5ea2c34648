// The host side of m4q_plant_robust_batch (csrc/m4q_robust_host.h) as a stand-alone program, built by
// tests/test_plant_robust_host.py with -fsanitize=address,undefined.
// argv[1]: a file of cases the test wrote, every number a C99 hexadecimal float (or inf):
//   <cases>
//   per case:  <nm> <mem> <steps> <sat> <step0>   U[nm]   g[nm]   <pairs> then s[nm] y[nm] per pair, oldest first
//              <pending> then, if 1, s_pend[nm] g_old[nm]
// Steps 2 - 5 of the loop run on each: project, absorb, direction, the candidates.  Printed per case, in hexadecimal floats:
//   K <pairs left>   G <gmax>   P p[nm]   C <j> candidate_j[nm] for every j
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "m4q_robust_host.h"

namespace rb = m4q::robust;

static bool number(std::istream& in, double& v) {
  std::string tok;
  if (!(in >> tok)) return false;
  char* end = nullptr;
  v = std::strtod(tok.c_str(), &end);
  return end != tok.c_str() && *end == '\0';
}

static bool vector(std::istream& in, size_t nm, rb::Vec& out) {
  out.resize(nm);
  for (size_t i = 0; i < nm; ++i)
    if (!number(in, out[i])) return false;
  return true;
}

static void print(const char* tag, const double* v, size_t nm) {
  std::printf("%s", tag);
  for (size_t i = 0; i < nm; ++i) std::printf(" %a", v[i]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  int cases = 0;
  if (!(in >> cases)) return 3;
  for (int c = 0; c < cases; ++c) {
    int nm = 0, steps = 0, pairs = 0, pending = 0;
    rb::State st;
    if (!(in >> nm >> st.mem >> steps) || nm < 1 || steps < 1 || !number(in, st.sat) || !number(in, st.step0)) return 4;
    if (!vector(in, nm, st.U) || !vector(in, nm, st.g) || !(in >> pairs) || pairs < 0) return 5;
    for (int q = 0; q < pairs; ++q) {
      rb::Pair pr;
      if (!vector(in, nm, pr.s) || !vector(in, nm, pr.y)) return 6;
      st.pairs.push_back(pr);
    }
    if (!(in >> pending)) return 7;
    if (pending) {
      if (!vector(in, nm, st.s_pend) || !vector(in, nm, st.g_old)) return 8;
      st.pending = true;
    }
    rb::project(st);
    rb::absorb(st);
    rb::direction(st);
    std::printf("K %zu\n", st.pairs.size());
    print("G", &st.gmax, 1);
    print("P", st.p.data(), st.p.size());
    rb::Vec cand(nm);
    for (int j = 0; j < steps; ++j) {
      rb::candidate(st, j, cand.data());
      std::printf("C %d", j);
      print("", cand.data(), cand.size());
    }
  }
  return 0;
}
