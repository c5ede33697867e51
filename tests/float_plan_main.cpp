// float_plan_main.cpp -- stand-alone driver of h-numo_amd/csrc/float_plan.h for tests/test_float_plan.py.
//
//   float_plan_main IN OUT
//
// IN and OUT are sequences of named records
//   int32 name length | name | 'i' (int32) or 'd' (float64) | int64 count | values
// (the format is private to the test).  IN: "ngl", "nelem", "nelem_owned", "nlayers", "nface", "face",
// "imapl", "imapr" (float_side_neighbours); then, unless "sides_only" = 1, "coord" + "ldc" + "xgl"
// (float_geometry), "xy" + "layer" + "M" (default: what xy holds; float_seed), and "dts" + "q": one
// float_advance_all per entry of dts, advance a on state min(a, S-1) of the S states q holds.  A pointer
// whose record is missing is NULL.  OUT: the tables, the permutation, the floats in input order after
// the last advance and "hist" (5, M, advances) = x, y, u, v, elem after each.  Exit status: 0 written,
// 3 the input was rejected (OUT holds the record "error"), 2 usage or I/O trouble.
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../h-numo_amd/csrc/float_plan.h"

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
static const int32_t *ip(const std::string &k) { return in.count(k) ? in[k].i.data() : nullptr; }
static const double *dp(const std::string &k) { return in.count(k) ? in[k].d.data() : nullptr; }
static int32_t iv(const std::string &k) { return in.count(k) && !in[k].i.empty() ? in[k].i[0] : 0; }

static FILE *out;
static void head(const std::string &name, char t, int64_t n) {
  const int32_t nl = (int32_t)name.size();
  fwrite(&nl, 4, 1, out);
  fwrite(name.data(), 1, nl, out);
  fwrite(&t, 1, 1, out);
  fwrite(&n, 8, 1, out);
}
static void put(const std::string &name, const std::vector<int32_t> &v) {
  head(name, 'i', (int64_t)v.size());
  if (!v.empty()) fwrite(v.data(), 4, v.size(), out);
}
static void put(const std::string &name, const std::vector<double> &v) {
  head(name, 'd', (int64_t)v.size());
  if (!v.empty()) fwrite(v.data(), 8, v.size(), out);
}
static int rejected(int rc, std::string err) {
  head("error", 'i', (int64_t)(err.size() + 3) / 4);  // (the text, zero-padded to whole words)
  err.resize((err.size() + 3) / 4 * 4, '\0');
  fwrite(err.data(), 1, err.size(), out);
  fclose(out);
  return rc == SP_ERR_INVALID ? 3 : 2;
}

template <class T>
static std::vector<T> unpermute(const std::vector<T> &v, const std::vector<int32_t> &perm) {
  std::vector<T> o(v.size());
  for (size_t s = 0; s < v.size(); s++) o[perm[s]] = v[s];
  return o;
}

int main(int argc, char **argv) {
  if (argc != 3 || !read_all(argv[1]) || !(out = fopen(argv[2], "wb"))) return 2;
  const int ngl = iv("ngl"), E = iv("nelem"), ne = iv("nelem_owned"), L = iv("nlayers"), F = iv("nface");
  std::string err;
  std::vector<int32_t> nbr;
  if (int rc = float_side_neighbours(ip("face"), ip("imapl"), ip("imapr"), F, ngl, E, ne, nbr, err)) return rejected(rc, err);
  put("nbr", nbr);
  if (iv("sides_only")) {
    fclose(out);
    return 0;
  }
  FloatGeom g;
  if (int rc = float_geometry(dp("coord"), iv("ldc"), dp("xgl"), ngl, ne, nbr, g, err)) return rejected(rc, err);
  int64_t M = (int64_t)in["xy"].d.size() / 2;
  if (in.count("M")) M = iv("M");
  FloatPlan p;
  if (int rc = float_seed(g, L, dp("xy"), ip("layer"), M, p, err)) return rejected(rc, err);
  put("maxc", std::vector<double>{g.maxc});
  put("corners", g.corners), put("tol", g.tol), put("perm", p.perm);
  put("elem0", unpermute(p.elem, p.perm)), put("status0", unpermute(p.status, p.perm));
  const std::vector<double> &dts = in["dts"].d, &q = in["q"].d;
  const size_t npoin = (size_t)E * ngl * ngl, nstate = 3 * npoin * (size_t)L;
  if (!dts.empty() && (nstate == 0 || q.size() < nstate || q.size() % nstate)) return 2;
  const size_t S = nstate ? q.size() / nstate : 0;
  std::vector<double> hist;
  for (size_t a = 0; a < dts.size(); a++) {
    float_advance_all(g, q.data() + std::min(a, S - 1) * nstate, npoin, dts[a], p);
    const std::vector<int32_t> el = unpermute(p.elem, p.perm);
    for (const std::vector<double> *v : {&p.x, &p.y, &p.wx, &p.wy}) {
      const std::vector<double> u = unpermute(*v, p.perm);
      hist.insert(hist.end(), u.begin(), u.end());
    }
    for (int32_t e : el) hist.push_back((double)e);
  }
  put("hist", hist);
  put("x", unpermute(p.x, p.perm)), put("y", unpermute(p.y, p.perm));
  put("wx", unpermute(p.wx, p.perm)), put("wy", unpermute(p.wy, p.perm));
  put("xi", unpermute(p.xi, p.perm)), put("eta", unpermute(p.eta, p.perm));
  put("elem", unpermute(p.elem, p.perm)), put("layer", unpermute(p.layer, p.perm));
  put("status", unpermute(p.status, p.perm)), put("fresh", unpermute(p.fresh, p.perm));
  fclose(out);
  return 0;
}
