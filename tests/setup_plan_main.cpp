// setup_plan_main.cpp -- stand-alone driver of h-numo_amd/csrc/setup_plan.h for tests/test_setup_plan.py.
//
//   setup_plan_main IN OUT
//
// IN is a descriptor dump, OUT receives the plan; both are sequences of named records
//   int32 name length | name | 'i' (int32) or 'd' (float64) | int64 count | values
// (the format is private to the test).  A pointer field whose record is missing is NULL, a scalar
// one 0; "null_mesh" / "null_statics" / "null_params" = 1 pass a NULL descriptor, "halo" = 1 passes
// a halo descriptor, "ncu" lists the CU counts to write placement_perm for ("perm_<ncu>").  Exit status: 0 plan written, 3 the
// descriptors were rejected (OUT holds the record "error"), 2 usage or I/O trouble.
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../h-numo_amd/csrc/setup_plan.h"

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
static double dv(const std::string &k) { return in.count(k) && !in[k].d.empty() ? in[k].d[0] : 0.0; }

static FILE *out;
static void head(const std::string &name, char t, int64_t n) {
  const int32_t nl = (int32_t)name.size();
  fwrite(&nl, 4, 1, out);
  fwrite(name.data(), 1, nl, out);
  fwrite(&t, 1, 1, out);
  fwrite(&n, 8, 1, out);
}
static void put(const std::string &name, const std::vector<int> &v) {
  head(name, 'i', (int64_t)v.size());
  if (!v.empty()) fwrite(v.data(), 4, v.size(), out);
}
static void put(const std::string &name, const std::vector<double> &v) {
  head(name, 'd', (int64_t)v.size());
  if (!v.empty()) fwrite(v.data(), 8, v.size(), out);
}

int main(int argc, char **argv) {
  if (argc != 3 || !read_all(argv[1]) || !(out = fopen(argv[2], "wb"))) return 2;
  hnumo_mesh_desc m{};
  m.nelem = iv("nelem"), m.npoin = iv("npoin"), m.npoin_q = iv("npoin_q"), m.nface = iv("nface");
  m.ngl = iv("ngl"), m.nq = iv("nq"), m.nlayers = iv("nlayers");
  m.face = ip("face"), m.imapl = ip("imapl"), m.imapr = ip("imapr"), m.imapl_q = ip("imapl_q"), m.imapr_q = ip("imapr_q");
  m.normal_vector = dp("normal_vector"), m.normal_vector_q = dp("normal_vector_q");
  m.jac_face = dp("jac_face"), m.jac_faceq = dp("jac_faceq"), m.massinv = dp("massinv");
  m.psiq = dp("psiq"), m.dpsiq = dp("dpsiq"), m.psi = dp("psi"), m.dpsi = dp("dpsi");
  m.ksiq_x = dp("ksiq_x"), m.ksiq_y = dp("ksiq_y"), m.etaq_x = dp("etaq_x"), m.etaq_y = dp("etaq_y"), m.jacq = dp("jacq");
  m.ksi_x = dp("ksi_x"), m.ksi_y = dp("ksi_y"), m.eta_x = dp("eta_x"), m.eta_y = dp("eta_y"), m.jac = dp("jac");
  hnumo_static_desc s{};
  s.pbprime = dp("s_pbprime"), s.pbprime_df = dp("s_pbprime_df"), s.one_over_pbprime = dp("s_one_over_pbprime");
  s.one_over_pbprime_df = dp("s_one_over_pbprime_df"), s.pbprime_face = dp("s_pbprime_face");
  s.pbprime_df_face = dp("s_pbprime_df_face"), s.one_over_pbprime_edge = dp("s_one_over_pbprime_edge");
  s.coeff_pbpert_L = dp("s_coeff_pbpert_L"), s.coeff_pbpert_R = dp("s_coeff_pbpert_R");
  s.coeff_pbub_LR = dp("s_coeff_pbub_LR"), s.coeff_mass_pbub_L = dp("s_coeff_mass_pbub_L");
  s.coeff_mass_pbub_R = dp("s_coeff_mass_pbub_R"), s.coeff_mass_pbpert_LR = dp("s_coeff_mass_pbpert_LR");
  s.alpha = dp("s_alpha"), s.tau_wind = dp("s_tau_wind"), s.coriolis_quad = dp("s_coriolis_quad");
  s.grad_zbot_quad = dp("s_grad_zbot_quad"), s.zbot_df = dp("s_zbot_df"), s.zbot_face = dp("s_zbot_face");
  s.fdt2_bcl = dp("s_fdt2_bcl"), s.a_bcl = dp("s_a_bcl"), s.b_bcl = dp("s_b_bcl");
  s.ssprk_a = dp("s_ssprk_a"), s.ssprk_beta = dp("s_ssprk_beta");
  hnumo_params p{};
  p.dt = dv("dt"), p.dt_btp = dv("dt_btp"), p.visc_mlswe = dv("visc_mlswe"), p.cd_mlswe = dv("cd_mlswe");
  p.ad_mlswe = dv("ad_mlswe"), p.gravity = dv("gravity"), p.max_shear_dz = dv("max_shear_dz");
  p.N_btp = iv("N_btp"), p.kstages = iv("kstages"), p.method_visc = iv("method_visc"), p.botfr = iv("botfr");
  p.shear_corrector = iv("shear_corrector");
  hnumo_halo_desc h{};
  h.rank = iv("rank"), h.nranks = iv("nranks"), h.num_nbh = iv("num_nbh"), h.nelem_owned = iv("nelem_owned");
  h.nbh_proc = ip("nbh_proc"), h.num_send_recv = ip("num_send_recv"), h.nbh_send_recv = ip("nbh_send_recv");
  h.num_ghost_send = ip("num_ghost_send"), h.ghost_send = ip("ghost_send");
  h.num_ghost_recv = ip("num_ghost_recv"), h.ghost_recv = ip("ghost_recv");

  SetupPlan pl;
  std::string err;
  const int rc = build_setup_plan(iv("null_mesh") ? nullptr : &m, iv("null_statics") ? nullptr : &s,
                                  iv("null_params") ? nullptr : &p, iv("halo") ? &h : nullptr, pl, err);
  if (rc != HNUMO_OK) {
    head("error", 'i', (int64_t)(err.size() + 3) / 4);  // (the text, zero-padded to whole words)
    err.resize((err.size() + 3) / 4 * 4, '\0');
    fwrite(err.data(), 1, err.size(), out);
    fclose(out);
    return rc == HNUMO_ERR_INVALID ? 3 : 2;
  }
  const int Q = m.nq * m.nq;
  std::vector<int> fnb, gnb_rank, gnb_nsend, gnb_nrecv, gnb_send, gnb_recv, qepos;
  for (const auto &n : pl.fnb) fnb.insert(fnb.end(), {n.rank, n.off, n.n});
  for (const auto &g : pl.gnb) {
    gnb_rank.push_back(g.rank);
    gnb_nsend.push_back((int)g.send.size());
    gnb_nrecv.push_back((int)g.recv.size());
    gnb_send.insert(gnb_send.end(), g.send.begin(), g.send.end());
    gnb_recv.insert(gnb_recv.end(), g.recv.begin(), g.recv.end());
  }
  for (int c = 0; c < QE_N; c++)
    for (int q = 0; q < Q; q++) qepos.push_back(qe_pos(c, q, Q));
  const SetupPlan::ConnOff &o = pl.off;
  put("scalars", std::vector<int>{pl.face_halo, pl.NS, pl.nelem_owned, (int)pl.nb0, EREC_SIZE(m.ngl), qe_stride(Q)});
  put("conn_off", std::vector<int>{(int)o.efaces, (int)o.eside, (int)o.ebc, (int)o.efmap, (int)o.enbr_node, (int)o.enbr_e,
                                   (int)o.enbr_lf, (int)o.fnodeL, (int)o.fnodeR, (int)o.fel, (int)o.fer, (int)o.fslotL,
                                   (int)o.fslotR, (int)o.fslotA, (int)o.erec});
  put("qe_pos", qepos);
  put("fnb", fnb), put("sface", pl.sface), put("face_slot", pl.face_slot);
  put("gnb_rank", gnb_rank), put("gnb_nsend", gnb_nsend), put("gnb_nrecv", gnb_nrecv);
  put("gnb_send", gnb_send), put("gnb_recv", gnb_recv);
  put("conn", pl.conn), put("fslotA", pl.fslotA), put("hb", pl.hb);
  put("qs", pl.qs), put("ns", pl.ns), put("fs", pl.fs), put("fns", pl.fns);
  put("qsE", pl.qsE), put("nsE", pl.nsE), put("efs", pl.efs);
  put("fq", pl.fq), put("tsrc", pl.tsrc), put("elB", pl.elB), put("elI", pl.elI);
  const int E = m.nelem;
  const std::vector<int> ebc(pl.conn.begin() + o.ebc, pl.conn.begin() + o.ebc + 4 * E);
  for (int ncu : in["ncu"].i) put("perm_" + std::to_string(ncu), placement_perm(ebc, E, ncu));
  fclose(out);
  return 0;
}
