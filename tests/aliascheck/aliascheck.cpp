// tests/aliascheck/aliascheck.cpp -- TEST INFRASTRUCTURE ONLY.
//
// Calls the product's fg_setup_group (ndpp_amd/csrc/fg_pipeline.h) on the CPU and checks the
// level-0 alias table it lays out (FgBatch::t_alias) against a brute-force look at the roots:
//   * an alias and its source belong to one job, both are live, their E_out are the same double;
//   * no source is itself an alias; only end points (slots 0 and 4) take part;
//   * an E_out held by two live end-point tasks of one job is aliased exactly once, and an E_out
//     held by one task never.
// usage: aliascheck A kT G bins[0] ... bins[G] ein[0] ein[1] ...
// prints "live_tasks N shared M aliases K" and exits 0, or a complaint and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../ndpp_amd/csrc/fg_pipeline.h"

using namespace ndpp;

static unsigned long long bits(double x) {
  unsigned long long u;
  memcpy(&u, &x, sizeof u);
  return u;
}

int main(int argc, char** argv) {
  if (argc < 6) { fprintf(stderr, "usage: see the source\n"); return 2; }
  const double A = atof(argv[1]), kT = atof(argv[2]);
  const int G = atoi(argv[3]);
  if (G < 1 || argc < 4 + G + 1 + 1) { fprintf(stderr, "expected %d group edges and an energy\n", G + 1); return 2; }
  std::vector<double> bins(G + 1), ein;
  for (int g = 0; g <= G; ++g) bins[g] = strtod(argv[4 + g], nullptr);
  for (int k = 4 + G + 1; k < argc; ++k) ein.push_back(strtod(argv[k], nullptr));

  FgBatch B{};
  B.n_jobs = (int)ein.size(); B.R = 2; B.G = G; B.L = 4; B.M = 0;
  B.A = A; B.kT = kT;
  B.job_ein = ein.data(); B.e_bins = bins.data();
  const int nt = B.n_trees();
  B.ncap = nt;
  std::vector<double> na(nt), nb(nt), nS((size_t)B.nch() * nt);
  std::vector<int> info((size_t)4 * nt), alias((size_t)5 * nt, -7);
  B.node_a = na.data(); B.node_b = nb.data(); B.node_S = nS.data(); B.node_info = info.data();
  B.tcap = 5 * nt;
  B.t_alias = alias.data();
  for (int j = 0; j < B.n_jobs; ++j)
    for (int g = 0; g < G; ++g) fg_setup_group(B, j, g);

  auto complain = [](const char* what, int t) { printf("FAIL: %s (task %d)\n", what, t); return 1; };
  auto live = [&](int n) { return B.node_info[4 * n + 0] != 0; };
  auto eout = [&](int t) { return fg_slot_point(B.node_a[t / 5], B.node_b[t / 5], t % 5); };
  long n_alias = 0, n_live = 0, n_shared = 0;
  for (int t = 0; t < 5 * nt; ++t) {
    const int src = alias[t];
    if (src == -7) return complain("entry never written", t);
    if (src < 0) continue;
    ++n_alias;
    if (src >= 5 * nt) return complain("source out of range", t);
    if (!live(t / 5) || !live(src / 5)) return complain("dead alias or source", t);
    if (B.node_job(t / 5) != B.node_job(src / 5)) return complain("alias and source in different jobs", t);
    if (bits(eout(t)) != bits(eout(src))) return complain("E_out differ", t);
    if (alias[src] >= 0) return complain("source is itself an alias", t);
    // (earlier along E_out: the source is the upper end of the segment below the alias's)
    if (t % 5 != 0 || src % 5 != 4) return complain("not a lower end aliased to an upper end", t);
  }
  // brute force, per job: the end-point tasks of live roots by the bits of their E_out
  for (int j = 0; j < B.n_jobs; ++j) {
    std::map<unsigned long long, std::vector<int>> by_e;
    for (int n = j * G * kSegPerGroup; n < (j + 1) * G * kSegPerGroup; ++n) {
      if (!live(n)) continue;
      if (bits(B.node_a[n]) == bits(B.node_b[n])) return complain("live zero-width root", 5 * n);
      n_live += 5;
      by_e[bits(B.node_a[n])].push_back(5 * n);
      by_e[bits(B.node_b[n])].push_back(5 * n + 4);
    }
    for (auto& kv : by_e) {
      int aliased = 0;
      for (int t : kv.second) aliased += alias[t] >= 0;
      if (kv.second.size() > 2) return complain("an E_out held by more than two end points", kv.second[0]);
      if (kv.second.size() == 2) {
        ++n_shared;
        if (aliased != 1) return complain("shared end point not aliased exactly once", kv.second[0]);
        const int t = alias[kv.second[0]] >= 0 ? kv.second[0] : kv.second[1];
        const int o = t == kv.second[0] ? kv.second[1] : kv.second[0];
        if (alias[t] != o) return complain("alias does not name the task that shares its E_out", t);
      } else if (aliased != 0) {
        return complain("lone end point aliased", kv.second[0]);
      }
    }
  }
  printf("live_tasks %ld shared %ld aliases %ld\n", n_live, n_shared, n_alias);
  return 0;
}
