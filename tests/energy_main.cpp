// energy_main.cpp -- stand-alone driver of the energy budget's host statements in h-numo_amd/csrc/energy_plan.h
// for tests/test_energy_plan.py.
//
//   energy_main IN OUT
//
// IN and OUT are sequences of named records as in tests/float_plan_main.cpp:
//   int32 name length | name | 'i' (int32) or 'd' (float64) | int64 count | values
// IN: "ngl", "nelem_owned", "nlayers", "botfr", "npoin", "npoin_q", "series" (0: sums only); "gravity", "cd", "visc";
//   "alpha", "zbot", optionally "zref" (npoin,L), "ksi_x", "ksi_y", "eta_x", "eta_y", "jac" (npoin), "wjac"
//   (npoin_q), "dpsi" ([m*ngl + i]), "psiq" ([m*nq + iq]); "q": one or more states q_df(3,npoin,L) one after the
//   other, "tau": as many winds tau_wind(2,npoin_q).  energy_host runs once per state on the same sums.
// OUT: "quad" (2,npoin_q), "nodal" (npoin,L); with a series "rows" (3L+2, states) and "part" (the last state's
//   element partials [3L+2][ne]).
// Exit status: 0 written, 3 the input was rejected, 2 usage or I/O trouble.
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../h-numo_amd/csrc/energy_plan.h"

using namespace hnumo;

struct Rec {
  std::vector<int32_t> i;
  std::vector<double> d;
};
static std::map<std::string, Rec> in;

static bool read_all(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  int32_t nl;
  while (fread(&nl, 4, 1, f) == 1) {
    std::string name(nl, ' ');
    char t;
    int64_t n;
    if (fread(&name[0], 1, nl, f) != (size_t)nl || fread(&t, 1, 1, f) != 1 || fread(&n, 8, 1, f) != 1) return false;
    Rec &r = in[name];
    if (t == 'i') {
      r.i.resize(n);
      if (n && fread(r.i.data(), 4, n, f) != (size_t)n) return false;
    } else {
      r.d.resize(n);
      if (n && fread(r.d.data(), 8, n, f) != (size_t)n) return false;
    }
  }
  fclose(f);
  return true;
}
static int32_t iv(const std::string &k) { return in.count(k) && !in[k].i.empty() ? in[k].i[0] : 0; }
static double dv(const std::string &k) { return in.count(k) && !in[k].d.empty() ? in[k].d[0] : 0.0; }
// the record's values when it holds exactly n of them
static const double *dp(const std::string &k, size_t n, bool &ok) {
  if (!in.count(k) || in[k].d.size() != n) {
    ok = false;
    return nullptr;
  }
  return in[k].d.data();
}

static FILE *out;
static void put(const std::string &name, const std::vector<double> &v) {
  const int32_t nl = (int32_t)name.size();
  const char t = 'd';
  const int64_t n = (int64_t)v.size();
  fwrite(&nl, 4, 1, out);
  fwrite(name.data(), 1, nl, out);
  fwrite(&t, 1, 1, out);
  fwrite(&n, 8, 1, out);
  if (!v.empty()) fwrite(v.data(), 8, v.size(), out);
}

int main(int argc, char **argv) {
  if (argc != 3 || !read_all(argv[1]) || !(out = fopen(argv[2], "wb"))) return 2;
  EnergyHost g{};
  g.ngl = iv("ngl"), g.ne = iv("nelem_owned"), g.L = iv("nlayers"), g.botfr = iv("botfr");
  g.npoin = (size_t)iv("npoin"), g.npq = (size_t)iv("npoin_q");
  g.gravity = dv("gravity"), g.cd = dv("cd"), g.visc = dv("visc");
  const int nq = 2 * g.ngl - 1, P = g.ngl * g.ngl, Q = nq * nq;
  if (g.ngl < 2 || g.L < 1 || g.L > EN_MAXL || g.ne < 0 || (size_t)g.ne * P > g.npoin || (size_t)g.ne * Q > g.npq) {
    fclose(out);
    return 3;
  }
  bool ok = true;
  const size_t nstate = 3 * g.npoin * g.L;
  g.alpha = dp("alpha", g.L, ok), g.zbot = dp("zbot", g.npoin, ok);
  g.zref = in.count("zref") ? dp("zref", g.npoin * g.L, ok) : nullptr;
  g.ex = dp("ksi_x", g.npoin, ok), g.ey = dp("ksi_y", g.npoin, ok), g.nx = dp("eta_x", g.npoin, ok), g.ny = dp("eta_y", g.npoin, ok);
  g.w = dp("jac", g.npoin, ok), g.wq = dp("wjac", g.npq, ok);
  g.dpsi = dp("dpsi", (size_t)P, ok), g.psiq = dp("psiq", (size_t)g.ngl * nq, ok);
  const std::vector<double> &qs = in["q"].d, &taus = in["tau"].d;
  const size_t ns = nstate ? qs.size() / nstate : 0;
  if (!ok || ns == 0 || qs.size() != ns * nstate || taus.size() != ns * 2 * g.npq) {
    fclose(out);
    return 3;
  }
  const bool series = iv("series") != 0;
  const int R = en_rows(g.L);
  std::vector<double> quad(2 * g.npq, 0.0), nodal(g.npoin * g.L, 0.0), rows, part(series ? (size_t)R * g.ne : 0);
  for (size_t s = 0; s < ns; s++) {
    g.q = qs.data() + s * nstate;
    g.tau = taus.data() + s * 2 * g.npq;
    std::vector<double> row(R);
    if (!energy_host(g, quad.data(), nodal.data(), series ? part.data() : nullptr, series ? row.data() : nullptr)) {
      fclose(out);
      return 3;
    }
    if (series) rows.insert(rows.end(), row.begin(), row.end());
  }
  put("quad", quad), put("nodal", nodal);
  if (series) put("rows", rows), put("part", part);
  fclose(out);
  return 0;
}
