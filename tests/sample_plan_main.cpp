// sample_plan_main.cpp -- stand-alone driver of h-numo_amd/csrc/sample_plan.h for tests/test_sample_plan.py.
//
//   sample_plan_main IN OUT
//
// IN and OUT are sequences of named records
//   int32 name length | name | 'i' (int32) or 'd' (float64) | int64 count | values
// (the format is private to the test).  IN: "ngl", "nelem_owned", "nlayers", "source", "M" (default:
// what xy / elem hold), "xgl", and either "coord" + "ldc" + "xy" (sample_locate) or "ref" = 1 + "elem"
// + "xi_eta" (sample_take_ref); a pointer whose record is missing is NULL.  OUT: the plan and its
// work lists.  Exit status: 0 plan written, 3 the input was rejected (OUT holds the record "error"),
// 2 usage or I/O trouble.
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../h-numo_amd/csrc/sample_plan.h"

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

int main(int argc, char **argv) {
  if (argc != 3 || !read_all(argv[1]) || !(out = fopen(argv[2], "wb"))) return 2;
  const int ngl = iv("ngl"), ne = iv("nelem_owned"), L = iv("nlayers"), source = iv("source");
  const bool ref = iv("ref") != 0;
  int64_t M = ref ? (int64_t)in["elem"].i.size() : (int64_t)in["xy"].d.size() / 2;
  if (in.count("M")) M = iv("M");
  SamplePlan pl;
  std::string err;
  const int rc = ref ? sample_take_ref(dp("xgl"), ngl, ne, ip("elem"), dp("xi_eta"), M, pl, err)
                     : sample_locate(dp("coord"), iv("ldc"), dp("xgl"), ngl, ne, dp("xy"), M, pl, err);
  if (rc != 0) {
    head("error", 'i', (int64_t)(err.size() + 3) / 4);  // (the text, zero-padded to whole words)
    err.resize((err.size() + 3) / 4 * 4, '\0');
    fwrite(err.data(), 1, err.size(), out);
    fclose(out);
    return rc == SP_ERR_INVALID ? 3 : 2;
  }
  const int V = sp_nval(L, source), K = sp_K(ngl, V);
  sample_chunks(dp("xgl"), K, pl);
  put("scalars", std::vector<int32_t>{K, V, sp_estride(ngl, V), SP_CHUNK, SP_LDS_BYTES, pl.nchunks()});
  put("maxc", std::vector<double>{pl.maxc});
  put("elem", pl.elem), put("xi_eta", pl.xi_eta);
  put("perm", pl.perm), put("slot", pl.slot), put("w", pl.w);
  put("chunk_pt", pl.chunk_pt), put("chunk_el", pl.chunk_el), put("el_list", pl.el_list);
  fclose(out);
  return 0;
}
