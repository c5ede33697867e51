// float_migrate_main.cpp -- stand-alone driver of the migrating float sets of h-numo_amd/csrc/float_plan.h for
// tests/test_float_migrate_plan.py: every rank of a processor-face partition in one process, through the
// header's advance / outbox / arrive statements -- the text the kernels run.
//
//   float_migrate_main IN OUT
//
// IN and OUT are sequences of named records as in tests/float_plan_main.cpp
//   int32 name length | name | 'i' (int32) or 'd' (float64) | int64 count | values
// IN: "nranks", "ngl", "nlayers", "ldc", "xgl", "xy", "layer", "dts", "scale" (coord_scale), and per rank r with
// the prefix "r<r>.": "nelem", "nface", "face", "imapl", "imapr", "coord", "q" (one state), "nbh_proc" (1-based),
// "num_send_recv", "nbh_send_recv" (1-based faces).  "tables_only" = 1: the tables alone.  A pointer whose record
// is missing is NULL.  OUT per rank: "nbr", "xface", "arrive", "released" (the seeds the lowest-rank rule released
// here) and "hist" (advances, 8, M) = x, y, wx, wy, xi, eta, elem, status after each advance, in input order; and
// "rounds" (advances), "inflight" (floats still in flight after the last round, summed).  Exit status: 0 written,
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

struct Rank {
  FloatGeom g;
  FloatPlan p;
  FloatRank t;
  std::vector<int32_t> nbh;  // 0-based neighbour ranks
  std::vector<FloatFlight> box, next;
  std::vector<double> hist;
  size_t npoin = 0;
};

int main(int argc, char **argv) {
  if (argc != 3 || !read_all(argv[1]) || !(out = fopen(argv[2], "wb"))) return 2;
  const int nr = iv("nranks"), ngl = iv("ngl"), L = iv("nlayers");
  const double scale = in.count("scale") && !in["scale"].d.empty() ? in["scale"].d[0] : 0.0;
  const int64_t M = (int64_t)in["xy"].d.size() / 2;
  if (nr < 1) return 2;
  std::vector<Rank> rk(nr);
  std::string err;
  for (int r = 0; r < nr; r++) {
    const std::string pre = "r" + std::to_string(r) + ".";
    Rank &R = rk[r];
    const int E = iv(pre + "nelem"), F = iv(pre + "nface");
    std::vector<int32_t> nbr;
    if (int rc = float_side_neighbours(ip(pre + "face"), ip(pre + "imapl"), ip(pre + "imapr"), F, ngl, E, E, nbr, err))
      return rejected(rc, err);
    const int nn = in.count(pre + "nbh_proc") ? (int)in[pre + "nbh_proc"].i.size() : iv(pre + "num_nbh");
    if (int rc = float_xface(ip(pre + "face"), ip(pre + "imapl"), F, ngl, E, nbr, nn, ip(pre + "num_send_recv"),
                             ip(pre + "nbh_send_recv"), R.t.xface, R.t.arrive, err))
      return rejected(rc, err);
    put(pre + "nbr", nbr), put(pre + "xface", R.t.xface), put(pre + "arrive", R.t.arrive);
    if (iv("tables_only")) continue;
    if (int rc = float_geometry(dp(pre + "coord"), iv("ldc"), dp("xgl"), ngl, E, nbr, R.g, err)) return rejected(rc, err);
    if (int rc = float_seed(R.g, L, dp("xy"), ip("layer"), M, R.p, err)) return rejected(rc, err);
    R.t.g = &R.g;
    R.t.tol = R.g.tol;
    if (scale > 0.0) float_tolerances(R.g.corners, scale, R.t.tol);
    R.t.iperm = float_inverse_perm(R.p.perm);
    int o = 0;
    for (int k = 0; k < nn; k++) {
      R.nbh.push_back(in[pre + "nbh_proc"].i[k] - 1);
      R.t.off.push_back(o);
      R.t.cnt.push_back(in[pre + "num_send_recv"].i[k]);
      o += R.t.cnt.back();
    }
    R.npoin = (size_t)E * ngl * ngl;
    if (in[pre + "q"].d.size() != 3 * R.npoin * (size_t)L) return 2;
  }
  if (iv("tables_only")) {
    fclose(out);
    return 0;
  }
  // a seed ACTIVE on several ranks stays on the lowest
  std::vector<char> held((size_t)M, 0);
  for (int r = 0; r < nr; r++) {
    Rank &R = rk[r];
    std::vector<int32_t> released;
    for (int64_t m = 0; m < M; m++) {
      const size_t s = (size_t)R.t.iperm[m];
      if (R.p.status[s] != FL_ACTIVE) continue;
      if (held[m]) {
        R.p.status[s] = FL_LEFT, R.p.elem[s] = 0, R.p.wx[s] = R.p.wy[s] = 0.0;
        released.push_back((int32_t)m);
      }
      held[m] = 1;
    }
    put("r" + std::to_string(r) + ".released", released);
  }
  const std::vector<double> &dts = in["dts"].d;
  std::vector<int32_t> rounds;
  int32_t inflight = 0;
  for (double dt : dts) {
    for (int r = 0; r < nr; r++) {
      Rank &R = rk[r];
      R.box.clear();
      const FloatField f = R.t.field(dp("r" + std::to_string(r) + ".q"), R.npoin);
      float_with_ngl(ngl, [&](auto n) { float_advance_mig_ngl<decltype(n)::value>(R.t, f, dt, R.p, R.box); });
    }
    int round = 0;
    for (;; round++) {
      size_t any = 0;
      for (const Rank &R : rk) any += R.box.size();
      if (!any) break;
      if (round == FL_MAXROUNDS) {
        for (Rank &R : rk)
          for (const FloatFlight &fl : R.box) R.p.status[(size_t)R.t.iperm[fl.gid]] = FL_LOST;
        inflight += (int32_t)any;
        break;
      }
      for (int r = 0; r < nr; r++) {
        Rank &R = rk[r];
        R.next.clear();
        const FloatField f = R.t.field(dp("r" + std::to_string(r) + ".q"), R.npoin);
        for (size_t k = 0; k < R.nbh.size(); k++) {
          const Rank &S = rk[R.nbh[k]];
          int me = -1;
          for (size_t j = 0; j < S.nbh.size(); j++)
            if (S.nbh[j] == r) me = (int)j;
          if (me < 0) continue;
          float_with_ngl(ngl, [&](auto n) { float_arrive_ngl<decltype(n)::value>(R.t, f, L, S.box, me, (int)k, R.p, R.next); });
        }
      }
      for (Rank &R : rk) R.box.swap(R.next);
    }
    rounds.push_back(round);
    for (Rank &R : rk) {
      const std::vector<double> *fd[6] = {&R.p.x, &R.p.y, &R.p.wx, &R.p.wy, &R.p.xi, &R.p.eta};
      for (int v = 0; v < 6; v++)
        for (int64_t m = 0; m < M; m++) R.hist.push_back((*fd[v])[(size_t)R.t.iperm[m]]);
      for (int64_t m = 0; m < M; m++) R.hist.push_back((double)R.p.elem[(size_t)R.t.iperm[m]]);
      for (int64_t m = 0; m < M; m++) R.hist.push_back((double)R.p.status[(size_t)R.t.iperm[m]]);
    }
  }
  for (int r = 0; r < nr; r++) put("r" + std::to_string(r) + ".hist", rk[r].hist);
  put("rounds", rounds);
  put("inflight", std::vector<int32_t>{inflight});
  fclose(out);
  return 0;
}
