// region_plan_main.cpp -- stand-alone driver of h-numo_amd/csrc/region_plan.h for tests/test_region_plan.py.
//
//   region_plan_main IN OUT
//
// IN and OUT are sequences of named records
//   int32 name length | name | 'i' (int32) or 'd' (float64) | int64 count | values
// (the format of tests/sample_plan_main.cpp).  IN: "labels" (missing: NULL), "n" (default: what labels
// holds), "nelem_owned", "R", "mask", and optionally "rows" with "part" [rows][nmem] for region_tree_host.
// OUT: the plan's tables, per pass the sizes and the descriptors (four int32 each), and "entry" [rows][R].
// Exit status: 0 plan written, 3 the input was rejected (OUT holds the record "error"), 2 usage or I/O
// trouble.
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../h-numo_amd/csrc/region_plan.h"

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
  const bool have = in.count("labels") != 0;
  static const int32_t none = 0;
  // (an empty label vector still gives a non-NULL pointer: NULL is its own case)
  const int32_t *labels = have ? (in["labels"].i.empty() ? &none : in["labels"].i.data()) : nullptr;
  const int64_t n = in.count("n") ? iv("n") : (int64_t)in["labels"].i.size();
  RegionPlan pl;
  std::string err;
  const int rc = region_plan(labels, n, iv("R"), iv("mask"), iv("nelem_owned"), pl, err);
  if (rc != 0) {
    head("error", 'i', (int64_t)(err.size() + 3) / 4);  // (the text, zero-padded to whole words)
    err.resize((err.size() + 3) / 4 * 4, '\0');
    fwrite(err.data(), 1, err.size(), out);
    fclose(out);
    return rc == RG_ERR_INVALID ? 3 : 2;
  }
  put("scalars", std::vector<int32_t>{pl.R, pl.mask, RG_CHUNK, RG_MAXSETS, (int32_t)pl.pass.size(), (int32_t)sizeof(RegionChunk)});
  put("members", pl.members), put("slot", pl.slot), put("offset", pl.offset);
  std::vector<int32_t> sizes, desc;
  for (const RegionPass &ps : pl.pass) {
    sizes.push_back((int32_t)ps.chunks.size());
    sizes.push_back((int32_t)ps.nin);
    sizes.push_back((int32_t)ps.nout);
    for (const RegionChunk &c : ps.chunks) desc.insert(desc.end(), {c.start, c.count, c.out, c.final});
  }
  put("pass_sizes", sizes), put("desc", desc);
  put("levels", std::vector<int32_t>{(int32_t)pl.level_size(0), (int32_t)pl.level_size(1)});
  if (const int rows = iv("rows"); rows > 0) {
    if ((int64_t)in["part"].d.size() != (int64_t)rows * pl.nmem()) return 2;
    std::vector<double> entry((size_t)rows * pl.R, -1.0);   // (every slot must be written)
    static const double nopart = 0.0;
    region_tree_host(pl, rows, in["part"].d.empty() ? &nopart : in["part"].d.data(), entry.data());
    put("entry", entry);
  }
  fclose(out);
  return 0;
}
