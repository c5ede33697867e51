// float_sense_main.cpp -- stand-alone driver of the sensors' host statements in h-numo_amd/csrc/float_plan.h for
// tests/test_float_sense_plan.py.
//
//   float_sense_main IN OUT
//
// IN and OUT are sequences of named records as in tests/float_plan_main.cpp:
//   int32 name length | name | 'i' (int32) or 'd' (float64) | int64 count | values
// Two uses.
//   "slot_elems" given: float_sense_slots over every block of "block" (default FL_BLOCK) consecutive entries.  OUT:
//     "slot" (one per entry), "nslots" (one per block), "list" (the blocks' lists, one after the other).
//   otherwise: the mesh and seeds of float_plan_main ("ngl", "nelem", "nelem_owned", "nlayers", "nface", "face",
//     "imapl", "imapr", "coord", "ldc", "xgl", "xy", "layer", "q", "dts") and the sensors' statics "zbot", "alpha",
//     "gravity", "ksi_x", "ksi_y", "eta_x", "eta_y", "dpsi" and optionally "f"; "mask"; "K" (a list; 0: the
//     kernel's).  After every advance float_sense_host runs once per entry of K.  OUT: "hist" (5, M, advances) and
//     "sense<i>" (S, M, advances) for the i-th entry of K, "K<i>" the K used, "elem_sorted" (M, advances): the
//     floats' elements in slot order.
// Exit status: 0 written, 3 the input was rejected (OUT holds the record "error"), 2 usage or I/O trouble.
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
  head("error", 'i', (int64_t)(err.size() + 3) / 4);
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

static int slots_only() {
  const std::vector<int32_t> &el = in["slot_elems"].i;
  const int block = in.count("block") ? iv("block") : FL_BLOCK;
  if (block < 1) return 2;
  std::vector<int32_t> slot(el.size()), nslots, lists;
  for (size_t b0 = 0; b0 < el.size(); b0 += block) {
    const int n = (int)std::min<size_t>(block, el.size() - b0);
    std::vector<int32_t> list(n);
    const int ns = float_sense_slots(el.data() + b0, n, slot.data() + b0, list.data());
    nslots.push_back(ns);
    lists.insert(lists.end(), list.begin(), list.begin() + ns);
  }
  put("slot", slot), put("nslots", nslots), put("list", lists);
  fclose(out);
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 3 || !read_all(argv[1]) || !(out = fopen(argv[2], "wb"))) return 2;
  if (in.count("slot_elems")) return slots_only();
  const int ngl = iv("ngl"), E = iv("nelem"), ne = iv("nelem_owned"), L = iv("nlayers"), F = iv("nface"), mask = iv("mask");
  std::string err;
  std::vector<int32_t> nbr;
  if (int rc = float_side_neighbours(ip("face"), ip("imapl"), ip("imapr"), F, ngl, E, ne, nbr, err)) return rejected(rc, err);
  FloatGeom g;
  if (int rc = float_geometry(dp("coord"), iv("ldc"), dp("xgl"), ngl, ne, nbr, g, err)) return rejected(rc, err);
  const int64_t M = (int64_t)in["xy"].d.size() / 2;
  FloatPlan p;
  if (int rc = float_seed(g, L, dp("xy"), ip("layer"), M, p, err)) return rejected(rc, err);
  if (L < 1 || L > 3 || mask < 1 || mask > FL_SENSE_ALL) return 2;
  const std::vector<double> &dts = in["dts"].d, &q = in["q"].d;
  const std::vector<int32_t> &Ks = in["K"].i;
  const size_t npoin = (size_t)E * ngl * ngl, nstate = 3 * npoin * (size_t)L;
  if (nstate == 0 || q.size() != nstate) return 2;
  for (const char *k : {"zbot", "ksi_x", "ksi_y", "eta_x", "eta_y"})
    if (in[k].d.size() != npoin) return 2;
  if (in["alpha"].d.size() < (size_t)L || in["gravity"].d.size() != 1 || in["dpsi"].d.size() != (size_t)ngl * ngl) return 2;
  if (in.count("f") && in["f"].d.size() != npoin) return 2;
  FloatSense fs{};
  fs.q = q.data();
  fs.zbot = dp("zbot"), fs.alpha = dp("alpha");
  fs.ex = dp("ksi_x"), fs.ey = dp("ksi_y"), fs.nx = dp("eta_x"), fs.ny = dp("eta_y");
  fs.f = dp("f");
  fs.dpsi = dp("dpsi");
  fs.gravity = in["gravity"].d[0];
  fs.npoin = npoin;
  for (int i = 0; i < ngl && i < 8; i++) fs.xgl[i] = g.xgl[i];
  const int S = fl_sense_rows(mask);
  std::vector<double> hist;
  std::vector<std::vector<double>> sense(Ks.size());
  std::vector<int32_t> elem_sorted;
  for (size_t a = 0; a < dts.size(); a++) {
    float_advance_all(g, q.data(), npoin, dts[a], p);
    for (const std::vector<double> *v : {&p.x, &p.y, &p.wx, &p.wy}) {
      const std::vector<double> u = unpermute(*v, p.perm);
      hist.insert(hist.end(), u.begin(), u.end());
    }
    for (int32_t e : unpermute(p.elem, p.perm)) hist.push_back((double)e);
    elem_sorted.insert(elem_sorted.end(), p.elem.begin(), p.elem.end());
    for (size_t t = 0; t < Ks.size(); t++) {
      std::vector<double> o((size_t)S * M, -7.0);
      float_sense_host(ngl, L, mask, fs, p, Ks[t], o.data());
      sense[t].insert(sense[t].end(), o.begin(), o.end());
    }
  }
  put("hist", hist);
  put("perm", p.perm);
  put("elem_sorted", elem_sorted);
  for (size_t t = 0; t < Ks.size(); t++) {
    put("sense" + std::to_string(t), sense[t]);
    int K = Ks[t];
    if (K <= 0)
      float_with_ngl(ngl, [&](auto n) {
        float_with_L_mask(L, mask, [&](auto l, auto m) { K = fl_sense_K(decltype(n)::value, decltype(l)::value, decltype(m)::value); });
      });
    put("K" + std::to_string(t), std::vector<int32_t>{K});
  }
  fclose(out);
  return 0;
}
