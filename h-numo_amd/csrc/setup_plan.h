// setup_plan.h -- the host-only half of engine creation: descriptor validation and every table
// the engine uploads, computed from the caller's arrays alone (no HIP call, no engine, no
// environment).  engine.hip includes it and uploads the plan; tests/setup_plan_main.cpp includes it
// and dumps the plan, so the tables the hand-written kernels index with are checked on the CPU
// (tests/test_setup_plan.py).  Loop orders and the order of the EF_PBLQ/EF_PBRQ sums are part of
// the bitwise contract.
#pragma once
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/hnumo_engine.h"
#include "engine_internal.h"

namespace hnumo {

static bool supported_ngl(int ngl) { return ngl == 3 || ngl == 4 || ngl == 5 || ngl == 6 || ngl == 8; }

struct SetupPlan {
  // processor-face halo: the reference's own partition contract (face(8) = 0 faces listed per
  // neighbour rank in nbh_send_recv; p4est.c:1686-1712, mod_parallel).  NS shared-face slots in
  // list order; neighbour j owns slots [off, off+n).
  bool face_halo = false;
  int NS = 0, nelem_owned = 0;
  struct FNbr {
    int rank = -1, off = 0, n = 0;
  };
  std::vector<FNbr> fnb;
  std::vector<int> sface;      // shared slot -> local face
  std::vector<int> face_slot;  // [F] local face -> shared slot (-1)
  // ghost-element halo: per neighbour its rank and the 0-based local element lists
  struct GNbr {
    int rank = -1;
    std::vector<int> send, recv;
  };
  std::vector<GNbr> gnb;
  // the int tables of DevMesh, concatenated in upload order
  struct ConnOff {
    size_t efaces, eside, ebc, efmap, enbr_node, enbr_e, enbr_lf, fnodeL, fnodeR, fel, fer, fslotL, fslotR, fslotA,
        erec;
  } off{};
  std::vector<int> conn;
  std::vector<int> fslotA;  // face -> slot holding its averages
  // basis: psiq, dpsiq [NGL*NQ], dpsi, psi [NGL*NGL], then at nb0 the stage kernel's interleaved copy
  std::vector<double> hb;
  size_t nb0 = 0;
  std::vector<double> qs, ns, fs, fns;  // SoA statics
  std::vector<double> qsE, nsE, efs;    // element-major statics (engine_internal.h)
  std::vector<int> fq;                  // method_visc == 1: [2][F][NQ] element-local quad point, left | right
  // processor-face halo: trace source slot of every element face; boundary / interior element lists
  std::vector<int> tsrc, elB, elI;
};

static int plan_fail(std::string &err, const char *msg) {
  err = msg;
  return HNUMO_ERR_INVALID;
}

// multi-rank: the reference's processor-face lists (num_send_recv / nbh_send_recv), or the
// ghost-element lists (num_ghost_send / num_ghost_recv) -- one of the two
// (nranks == 1 with processor-face lists: the self-neighbour test contract -- every listed face
// is shared with this rank itself, so each receives its own side 1 as side 2 over the same
// transport code as a real neighbour's; tests/test_rccl_self_gpu.py)
static int plan_halo_lists(const hnumo_mesh_desc *mesh, const hnumo_halo_desc *halo, SetupPlan &pl, std::string &err) {
  std::vector<int> &sface = pl.sface, &face_slot = pl.face_slot;
  face_slot.assign(mesh->nface > 0 ? mesh->nface : 0, -1);
  if (halo && (halo->nranks > 1 || halo->num_nbh > 0)) {
    if (halo->rank < 0 || halo->rank >= halo->nranks) return plan_fail(err, "bad rank");
    bool any_face = false, any_ghost = false;
    for (int k = 0; k < halo->num_nbh; k++) {
      if (halo->num_send_recv && halo->num_send_recv[k] > 0) any_face = true;
      if ((halo->num_ghost_send && halo->num_ghost_send[k] > 0) || (halo->num_ghost_recv && halo->num_ghost_recv[k] > 0))
        any_ghost = true;
    }
    if (any_face && any_ghost)
      return plan_fail(err, "give either processor-face lists or ghost-element lists, not both");
    if (any_face) {
      pl.face_halo = true;
      if (halo->nelem_owned != 0 && halo->nelem_owned != mesh->nelem)
        return plan_fail(err, "processor-face halo: every local element is owned (nelem_owned = nelem)");
      if (!halo->nbh_proc || !halo->num_send_recv || !halo->nbh_send_recv)
        return plan_fail(err, "processor-face halo needs nbh_proc, num_send_recv, nbh_send_recv");
      size_t o = 0;
      for (int k = 0; k < halo->num_nbh; k++) {
        SetupPlan::FNbr nb;
        nb.rank = halo->nbh_proc[k] - 1;  // mod_parallel nbh_proc is 1-based (p4est.c:1357)
        nb.off = (int)sface.size();
        nb.n = halo->num_send_recv[k];
        if (nb.rank < 0 || nb.rank >= halo->nranks || (nb.rank == halo->rank && halo->nranks > 1))
          return plan_fail(err, "nbh_proc: bad neighbour rank (1-based ranks expected)");
        // mod_parallel lists each neighbour process once (p4est.c:1343-1360); the transports pair a
        // rank's message with the peer's one entry for it.  The one exception is the self-neighbour
        // contract (nranks == 1): a W-rank partition's rank emulated on one GPU may keep its real
        // per-neighbour lists, every one addressed to itself -- one ncclSend/ncclRecv pair per list
        // inside the group (RCCL matches same-peer operations in issue order), each list's message
        // at its own offset and size, as on the W-GPU run
        if (halo->nranks > 1)
          for (const auto &pn : pl.fnb)
            if (pn.rank == nb.rank) return plan_fail(err, "nbh_proc: a neighbour rank is listed twice");
        if (nb.n < 0) return plan_fail(err, "num_send_recv < 0");
        for (int i = 0; i < nb.n; i++) {
          const int f = halo->nbh_send_recv[o + i] - 1;
          if (f < 0 || f >= mesh->nface) return plan_fail(err, "nbh_send_recv: face id out of range");
          if (mesh->face[8 * f + 7] != 0)
            return plan_fail(err, "nbh_send_recv lists a face whose face(8) is not 0 (not a processor face)");
          if (face_slot[f] >= 0)
            return plan_fail(err, "a processor face is listed twice (non-conforming multiplicity > 1 is not supported)");
          face_slot[f] = (int)sface.size();
          sface.push_back(f);
        }
        o += nb.n;
        pl.fnb.push_back(nb);
      }
      pl.NS = (int)sface.size();
    } else {
      if (halo->nranks < 2) return plan_fail(err, "ghost-element lists need nranks > 1");
      if (halo->nelem_owned < 1 || halo->nelem_owned > mesh->nelem)
        return plan_fail(err, "nelem_owned must be in 1..nelem (owned elements first)");
    }
  }
  return HNUMO_OK;
}

// the ghost-element halo's per-neighbour lists, 0-based
static int plan_ghost_lists(const hnumo_mesh_desc *mesh, const hnumo_halo_desc *halo, SetupPlan &pl, std::string &err) {
  const int E = mesh->nelem;
  size_t os = 0, orr = 0;
  for (int k = 0; k < halo->num_nbh; k++) {
    SetupPlan::GNbr nb;
    nb.rank = halo->nbh_proc[k];
    const int nsend = halo->num_ghost_send ? halo->num_ghost_send[k] : 0;
    const int nrecv = halo->num_ghost_recv ? halo->num_ghost_recv[k] : 0;
    if (nb.rank < 0 || nb.rank >= halo->nranks || nb.rank == halo->rank) return plan_fail(err, "bad neighbour rank");
    for (const auto &pn : pl.gnb)
      if (pn.rank == nb.rank) return plan_fail(err, "a neighbour rank is listed twice");
    std::vector<int> &snd = nb.send, &rcv = nb.recv;
    snd.resize(nsend > 0 ? nsend : 0);
    rcv.resize(nrecv > 0 ? nrecv : 0);
    for (int i = 0; i < nsend; i++) {
      snd[i] = halo->ghost_send[os + i] - 1;
      if (snd[i] < 0 || snd[i] >= pl.nelem_owned) return plan_fail(err, "ghost_send must list owned elements");
    }
    for (int i = 0; i < nrecv; i++) {
      rcv[i] = halo->ghost_recv[orr + i] - 1;
      if (rcv[i] < pl.nelem_owned || rcv[i] >= E) return plan_fail(err, "ghost_recv must list ghost elements");
    }
    os += snd.size();
    orr += rcv.size();
    pl.gnb.push_back(std::move(nb));
  }
  return HNUMO_OK;
}

// element -> face connectivity from the reference face arrays, the per-element int records of
// the stage kernel, and (processor-face halo) the trace source slots and element lists
static int plan_connectivity(const hnumo_mesh_desc *mesh, SetupPlan &pl, std::string &err) {
  const int E = mesh->nelem, ngl = mesh->ngl, F = mesh->nface, P = ngl * ngl, EO = pl.nelem_owned;
  const size_t FN = (size_t)F * ngl;
  const std::vector<int> &face_slot = pl.face_slot;
  std::vector<std::vector<std::pair<int, int>>> ef(E);
  for (int f = 0; f < F; f++) {
    int el = mesh->face[8 * f + 6] - 1, er = mesh->face[8 * f + 7];
    if (el < 0 || el >= E) return plan_fail(err, "face(7) out of range");
    ef[el].push_back({f, 0});
    if (er > 0) {
      if (er > E) return plan_fail(err, "face(8) out of range");
      ef[er - 1].push_back({f, 1});
    } else if (er == 0 && face_slot[f] < 0) {
      return plan_fail(err, "face(8) = 0 (processor face) but the face is not in the halo's nbh_send_recv lists");
    }
  }
  auto lnode = [&](const int32_t *imap, int f, int n) {
    int i = imap[3 * (n + ngl * f)] - 1, j = imap[3 * (n + ngl * f) + 1] - 1;
    return j * ngl + i;
  };
  std::vector<int> efaces(4 * E), eside(4 * E), ebc(4 * E), efmap(4 * E * ngl), enbr_node(4 * E * ngl, -1);
  std::vector<int> enbr_e(4 * E, -1), enbr_lf(4 * E, -1), fnodeL(FN), fnodeR(FN, -1), fel(F), fer(F);
  for (int e = 0; e < E; e++) {
    if (ef[e].size() != 4) return plan_fail(err, "every element needs exactly 4 faces");
    std::sort(ef[e].begin(), ef[e].end());
  }
  for (int e = 0; e < E; e++)
    for (int lf = 0; lf < 4; lf++) {
      int f = ef[e][lf].first, s = ef[e][lf].second;
      int el = mesh->face[8 * f + 6] - 1, er = mesh->face[8 * f + 7];
      efaces[4 * e + lf] = f;
      eside[4 * e + lf] = s;
      ebc[4 * e + lf] = er;
      for (int n = 0; n < ngl; n++) efmap[(4 * e + lf) * ngl + n] = lnode(s == 0 ? mesh->imapl : mesh->imapr, f, n);
      if (er > 0) {
        int nb = s == 0 ? er - 1 : el;
        enbr_e[4 * e + lf] = nb;
        for (int k = 0; k < 4; k++)
          if (ef[nb][k].first == f) enbr_lf[4 * e + lf] = k;
        for (int n = 0; n < ngl; n++)
          enbr_node[(4 * e + lf) * ngl + n] = nb * P + lnode(s == 0 ? mesh->imapr : mesh->imapl, f, n);
      } else if (er == 0) {
        // processor face: the stage writes this face's traces into send slot 4E + s of the
        // trace buffer, i.e. "element" E + s/4, local face s%4
        const int sl = face_slot[f];
        enbr_e[4 * e + lf] = E + sl / 4;
        enbr_lf[4 * e + lf] = sl % 4;
      }
    }
  for (int f = 0; f < F; f++) {
    int el = mesh->face[8 * f + 6] - 1, er = mesh->face[8 * f + 7];
    fel[f] = el;
    fer[f] = er;
    for (int n = 0; n < ngl; n++) {
      fnodeL[(size_t)f * ngl + n] = el * P + lnode(mesh->imapl, f, n);
      if (er > 0) fnodeR[(size_t)f * ngl + n] = (er - 1) * P + lnode(mesh->imapr, f, n);
    }
  }
  // face -> element-side slots; per-element int records for the stage kernel
  std::vector<int> fslotL(F, -1), fslotR(F, -1), fslotA(F, -1);
  for (int e = 0; e < E; e++)
    for (int lf = 0; lf < 4; lf++) (eside[4 * e + lf] == 0 ? fslotL : fslotR)[efaces[4 * e + lf]] = 4 * e + lf;
  // face averages are kept by the left element, or by the right one when the left is a ghost
  for (int f = 0; f < F; f++) {
    const int el = fel[f], er = fer[f];
    fslotA[f] = (el >= EO && er > 0 && er - 1 < EO) ? fslotR[f] : fslotL[f];
  }
  const int ERS = EREC_SIZE(ngl);
  std::vector<int> erec((size_t)E * ERS, -1);
  for (int e = 0; e < E; e++) {
    int *r = &erec[(size_t)e * ERS];
    for (int lf = 0; lf < 4; lf++) {
      r[EREC_FACE + lf] = efaces[4 * e + lf];
      r[EREC_SIDE + lf] = eside[4 * e + lf];
      r[EREC_BC + lf] = ebc[4 * e + lf];
      r[EREC_NBE + lf] = enbr_e[4 * e + lf];
      r[EREC_NBLF + lf] = enbr_lf[4 * e + lf];
      r[EREC_ACC + lf] = fslotA[efaces[4 * e + lf]] == 4 * e + lf ? 1 : 0;
      for (int n = 0; n < ngl; n++) r[EREC_MAP + lf * ngl + n] = efmap[(4 * e + lf) * ngl + n];
      if (ebc[4 * e + lf] > 0) {
        // the stage kernel writes face traces into the neighbour's slot with the same face-node index
        const int nb = enbr_e[4 * e + lf], nlf = enbr_lf[4 * e + lf];
        for (int n = 0; n < ngl; n++)
          if (enbr_node[(4 * e + lf) * ngl + n] != nb * P + efmap[(4 * nb + nlf) * ngl + n])
            return plan_fail(err, "face node orderings of neighbouring elements disagree");
      }
    }
    for (int lf = 0; lf < 4; lf++)
      for (int n = 0; n < ngl; n++) {
        int *pf = &r[EREC_PF(ngl) + 2 * efmap[(4 * e + lf) * ngl + n]];
        if (pf[0] < 0) pf[0] = lf * ngl + n; else if (pf[1] < 0) pf[1] = lf * ngl + n;
        else return plan_fail(err, "a node lies on more than two faces of its element");
      }
  }
  pl.fslotA = fslotA;
  std::vector<int> &conn = pl.conn;
  auto append = [&](const std::vector<int> &v) {
    size_t off = conn.size();
    conn.insert(conn.end(), v.begin(), v.end());
    return off;
  };
  SetupPlan::ConnOff &o = pl.off;
  o.efaces = append(efaces), o.eside = append(eside), o.ebc = append(ebc), o.efmap = append(efmap);
  o.enbr_node = append(enbr_node), o.enbr_e = append(enbr_e), o.enbr_lf = append(enbr_lf), o.fnodeL = append(fnodeL);
  o.fnodeR = append(fnodeR), o.fel = append(fel), o.fer = append(fer);
  o.fslotL = append(fslotL), o.fslotR = append(fslotR), o.fslotA = append(fslotA), o.erec = append(erec);
  if (pl.face_halo) {
    const int NS = pl.NS;
    std::vector<int> &tsrc = pl.tsrc, &elB = pl.elB, &elI = pl.elI;
    tsrc.resize(4 * (size_t)E);
    for (int e = 0; e < E; e++) {
      bool bnd = false;
      for (int lf = 0; lf < 4; lf++) {
        const int f = efaces[4 * e + lf];
        const bool proc = ebc[4 * e + lf] == 0;
        tsrc[4 * e + lf] = proc ? 4 * E + NS + face_slot[f] : 4 * e + lf;
        bnd |= proc;
      }
      (bnd ? elB : elI).push_back(e);
    }
  }
  return HNUMO_OK;
}

// the basis layouts and the SoA statics blocks
static int plan_statics(const hnumo_mesh_desc *mesh, const hnumo_static_desc *st, SetupPlan &pl, std::string &err) {
  const int E = mesh->nelem, ngl = mesh->ngl, nq = mesh->nq, F = mesh->nface;
  const size_t npoin = (size_t)E * ngl * ngl, npq = (size_t)E * nq * nq, FQ = (size_t)F * nq, FN = (size_t)F * ngl;
  // (+ the stage kernel's interleaved copy, basis_pd: 16-byte aligned, the counts above are even)
  const size_t nb0 = pl.nb0 = 2 * (size_t)ngl * nq + 2 * (size_t)ngl * ngl;
  std::vector<double> &hb = pl.hb;
  hb.assign(nb0 + 2 * ngl * nq + ngl * ngl, 0.0);
  for (int n = 0; n < ngl; n++)
    for (int iq = 0; iq < nq; iq++) {
      hb[n * nq + iq] = mesh->psiq[n + ngl * iq];
      hb[ngl * nq + n * nq + iq] = mesh->dpsiq[n + ngl * iq];
    }
  for (int n = 0; n < ngl; n++)
    for (int k = 0; k < ngl; k++) {
      hb[2 * ngl * nq + n * ngl + k] = mesh->dpsi[n + ngl * k];
      hb[2 * ngl * nq + ngl * ngl + n * ngl + k] = mesh->psi[n + ngl * k];
    }
  for (int x = 0; x < ngl * nq; x++) {
    hb[nb0 + 2 * x] = hb[x];
    hb[nb0 + 2 * x + 1] = hb[ngl * nq + x];
  }
  for (int x = 0; x < ngl * ngl; x++) hb[nb0 + 2 * ngl * nq + x] = hb[2 * ngl * nq + x];
  // the stage kernels drop the zero terms of the nodal derivative sums: psi must be the
  // identity at the LGL nodes (it is, exactly, for the reference's nodal basis)
  for (int n = 0; n < ngl; n++)
    for (int k = 0; k < ngl; k++)
      if (mesh->psi[n + ngl * k] != (n == k ? 1.0 : 0.0))
        return plan_fail(err, "nodal basis psi is not the identity at the LGL nodes");
  std::vector<double> &qs = pl.qs, &ns = pl.ns, &fs = pl.fs, &fns = pl.fns;
  qs.assign(QS_N * npq, 0.0), ns.assign(NS_N * npoin, 0.0), fs.assign(FS_N * FQ, 0.0), fns.assign(FN_N * FN, 0.0);
  for (size_t i = 0; i < npq; i++) {
    qs[QS_W * npq + i] = mesh->jacq[i];
    qs[QS_COR * npq + i] = st->coriolis_quad[i];
    qs[QS_TW1 * npq + i] = st->tau_wind[2 * i];
    qs[QS_TW2 * npq + i] = st->tau_wind[2 * i + 1];
    qs[QS_GZ1 * npq + i] = st->grad_zbot_quad[2 * i];
    qs[QS_GZ2 * npq + i] = st->grad_zbot_quad[2 * i + 1];
    qs[QS_OOP * npq + i] = st->one_over_pbprime[i];
    qs[QS_EX * npq + i] = mesh->ksiq_x[i];
    qs[QS_EY * npq + i] = mesh->ksiq_y[i];
    qs[QS_NX * npq + i] = mesh->etaq_x[i];
    qs[QS_NY * npq + i] = mesh->etaq_y[i];
    qs[QS_PB * npq + i] = st->pbprime[i];
  }
  for (size_t i = 0; i < npoin; i++) {
    ns[NS_PB * npoin + i] = st->pbprime_df[i];
    ns[NS_OOP * npoin + i] = st->one_over_pbprime_df[i];
    ns[NS_MINV * npoin + i] = mesh->massinv[i];
    ns[NS_W * npoin + i] = mesh->jac[i];
    ns[NS_EX * npoin + i] = mesh->ksi_x[i];
    ns[NS_EY * npoin + i] = mesh->ksi_y[i];
    ns[NS_NX * npoin + i] = mesh->eta_x[i];
    ns[NS_NY * npoin + i] = mesh->eta_y[i];
    ns[NS_ZB * npoin + i] = st->zbot_df[i];
    ns[NS_F2 * npoin + i] = st->fdt2_bcl[i];
    ns[NS_A * npoin + i] = st->a_bcl[i];
    ns[NS_B * npoin + i] = st->b_bcl[i];
  }
  for (size_t i = 0; i < FQ; i++) {
    fs[FS_NX * FQ + i] = mesh->normal_vector_q[3 * i];
    fs[FS_NY * FQ + i] = mesh->normal_vector_q[3 * i + 1];
    fs[FS_W * FQ + i] = mesh->jac_faceq[i];
    fs[FS_CL * FQ + i] = st->coeff_pbpert_L[i];
    fs[FS_CR * FQ + i] = st->coeff_pbpert_R[i];
    fs[FS_CLR * FQ + i] = st->coeff_pbub_LR[i];
    fs[FS_CML * FQ + i] = st->coeff_mass_pbub_L[i];
    fs[FS_CMR * FQ + i] = st->coeff_mass_pbub_R[i];
    fs[FS_CMLR * FQ + i] = st->coeff_mass_pbpert_LR[i];
    fs[FS_OOPE * FQ + i] = st->one_over_pbprime_edge[i];
    fs[FS_PBL * FQ + i] = st->pbprime_face[2 * i];
    fs[FS_PBR * FQ + i] = st->pbprime_face[2 * i + 1];
    fs[FS_ZBL * FQ + i] = st->zbot_face[2 * i];
    fs[FS_ZBR * FQ + i] = st->zbot_face[2 * i + 1];
  }
  for (size_t i = 0; i < FN; i++) {
    fns[FN_NX * FN + i] = mesh->normal_vector[3 * i];
    fns[FN_NY * FN + i] = mesh->normal_vector[3 * i + 1];
    fns[FN_W * FN + i] = mesh->jac_face[i];
    fns[FN_PBL * FN + i] = st->pbprime_df_face[2 * i];
    fns[FN_PBR * FN + i] = st->pbprime_df_face[2 * i + 1];
  }
  return HNUMO_OK;
}

// element-major statics (engine_internal.h)
static void plan_element_major(const hnumo_mesh_desc *mesh, SetupPlan &plan) {
  const int E = mesh->nelem, ngl = mesh->ngl, nq = mesh->nq, F = mesh->nface, P = ngl * ngl;
  const size_t npoin = (size_t)E * P, npq = (size_t)E * nq * nq, FQ = (size_t)F * nq, FN = (size_t)F * ngl;
  const int *efaces = &plan.conn[plan.off.efaces];
  const std::vector<double> &hb = plan.hb, &qs = plan.qs, &ns = plan.ns, &fs = plan.fs, &fns = plan.fns;
  std::vector<double> &qsE = plan.qsE, &nsE = plan.nsE, &efs = plan.efs;
  const int Qe = nq * nq, FBLK = EF_N * nq + EFN_N * ngl;
  qsE.assign((size_t)E * qe_stride(Qe), 0.0), nsE.assign((size_t)E * NE_N * P, 0.0), efs.assign((size_t)E * 4 * FBLK, 0.0);
  const int qmap[QE_N] = {QS_W, QS_EX, QS_EY, QS_NX, QS_NY, QS_COR, QS_TW1, QS_TW2, QS_GZ1, QS_GZ2, QS_OOP};
  const int nmap[NE_N] = {NS_EX, NS_EY, NS_NX, NS_NY, NS_W, NS_OOP, NS_MINV, NS_PB};
  const int fmap_[EF_PBLQ] = {FS_NX, FS_NY, FS_W, FS_CL, FS_CR, FS_CLR, FS_CML, FS_CMR, FS_CMLR, FS_OOPE};
  const int fnmap[EFN_N] = {FN_NX, FN_NY, FN_W, FN_PBL, FN_PBR};
  for (int e = 0; e < E; e++) {
    for (int c = 0; c < QE_N; c++)
      for (int q = 0; q < Qe; q++) qsE[(size_t)e * qe_stride(Qe) + qe_pos(c, q, Qe)] = qs[qmap[c] * npq + (size_t)e * Qe + q];
    for (int c = 0; c < NE_N; c++)
      for (int p = 0; p < P; p++) nsE[((size_t)e * NE_N + c) * P + p] = ns[nmap[c] * npoin + (size_t)e * P + p];
    for (int lf = 0; lf < 4; lf++) {
      const size_t f = efaces[4 * e + lf];
      double *b = &efs[((size_t)e * 4 + lf) * FBLK];
      for (int c = 0; c < EF_PBLQ; c++)
        for (int iq = 0; iq < nq; iq++) b[c * nq + iq] = fs[fmap_[c] * FQ + f * nq + iq];
      // creat_btp_fluxes_qdf's pbl/pbr (mod_rhs_btp.F90:255-258): same products, same order
      for (int iq = 0; iq < nq; iq++) {
        double pl = 0.0, pr = 0.0;
        for (int n = 0; n < ngl; n++) {
          pl = pl + hb[n * nq + iq] * fns[FN_PBL * FN + f * ngl + n];
          pr = pr + hb[n * nq + iq] * fns[FN_PBR * FN + f * ngl + n];
        }
        b[EF_PBLQ * nq + iq] = pl;
        b[EF_PBRQ * nq + iq] = pr;
      }
      for (int c = 0; c < EFN_N; c++)
        for (int n = 0; n < ngl; n++) b[EF_N * nq + c * ngl + n] = fns[fnmap[c] * FN + f * ngl + n];
    }
  }
}

// method_visc == 1 (quad-point LDG, kernels_lapq.hip): element-local quad point of every face quad point
static int plan_fq(const hnumo_mesh_desc *mesh, SetupPlan &pl, std::string &err) {
  const int nq = mesh->nq, F = mesh->nface;
  const size_t FQ = (size_t)F * nq;
  std::vector<int> &fq = pl.fq;
  fq.assign(2 * FQ, -1);
  for (int s = 0; s < 2; s++) {
    const int32_t *imq = s == 0 ? mesh->imapl_q : mesh->imapr_q;
    for (int f = 0; f < F; f++)
      for (int iq = 0; iq < nq; iq++) {
        const int i = imq[3 * (iq + nq * f)] - 1, j = imq[3 * (iq + nq * f) + 1] - 1;
        if (s == 1 && mesh->face[8 * f + 7] <= 0) continue;
        if (i < 0 || i >= nq || j < 0 || j >= nq) return plan_fail(err, "imapl_q/imapr_q out of range");
        fq[s * FQ + (size_t)f * nq + iq] = j * nq + i;
      }
  }
  return HNUMO_OK;
}

// Validates the descriptors and fills the plan: HNUMO_OK, or HNUMO_ERR_INVALID with the message
// in err.  The checks run in a fixed order; the first failure is the one reported.
static int build_setup_plan(const hnumo_mesh_desc *mesh, const hnumo_static_desc *st, const hnumo_params *par,
                            const hnumo_halo_desc *halo, SetupPlan &pl, std::string &err) {
  if (!mesh || !st || !par) return plan_fail(err, "null descriptor");
  if (int rc = plan_halo_lists(mesh, halo, pl, err)) return rc;
  const bool ghosts = halo && halo->nranks > 1 && !pl.face_halo;
  if (par->method_visc == 1) {
    if (!mesh->imapl_q || !mesh->imapr_q) return plan_fail(err, "method_visc==1 needs imapl_q/imapr_q");
    if (ghosts)
      return plan_fail(err, "method_visc==1 (quad-point LDG) runs on one rank or on the processor-face halo, not on ghost elements");
  }
  if (par->shear_corrector != HNUMO_SHEAR_CORRECTOR_REFERENCE && par->shear_corrector != HNUMO_SHEAR_CORRECTOR_PREDICTED)
    return plan_fail(err, "shear_corrector must be HNUMO_SHEAR_CORRECTOR_REFERENCE or _PREDICTED");
  if (mesh->nlayers < 1 || mesh->nlayers > MAXL)
    return plan_fail(err, "nlayers must be 1..3 (qp(k) quirk, mod_create_rhs_mlswe.F90:382)");
  if (!supported_ngl(mesh->ngl) || mesh->nq != 2 * mesh->ngl - 1)
    return plan_fail(err, "unsupported polynomial order (N in {2,3,4,5,7}, nq=2N+1)");
  if (par->kstages < 1 || par->kstages > 5 || par->N_btp < 1) return plan_fail(err, "bad kstages/N_btp");
  const int E = mesh->nelem, P = mesh->ngl * mesh->ngl, Q = mesh->nq * mesh->nq;
  if (mesh->npoin != E * P || mesh->npoin_q != E * Q) return plan_fail(err, "npoin/npoin_q mismatch");
  pl.nelem_owned = ghosts ? halo->nelem_owned : E;
  if (int rc = plan_connectivity(mesh, pl, err)) return rc;
  if (int rc = plan_statics(mesh, st, pl, err)) return rc;
  plan_element_major(mesh, pl);
  if (par->method_visc == 1)
    if (int rc = plan_fq(mesh, pl, err)) return rc;
  if (ghosts)
    if (int rc = plan_ghost_lists(mesh, halo, pl, err)) return rc;
  return HNUMO_OK;
}

// The persistent sub-cycle's workgroup -> element placement on ncu compute units (empty: the
// identity).  Workgroup b runs on CU b % ncu (the dispatcher's round-robin; blocks b,
// b + ncu, b + 2 ncu share a CU), so with E/ncu not whole some CUs hold one element more; the
// elements with a physical-boundary face (more work: ghost states, wall fluxes) go to the CUs
// holding fewer, the others fill the rest in order.  Same arithmetic per element, same bits
// (dg25L3: 16 us less sub-cycle time per step in 3 interleaved pairs, profiles/r05x).
static std::vector<int> placement_perm(const std::vector<int> &ebc, int E, int ncu) {
  if (ncu <= 0 || E % ncu == 0) return {};
  const int nheavy = E % ncu;  // CUs k < nheavy hold one block more
  // (measured, not kept: also grouping by XCD -- blocks b and b + 8 share one, so group b % 8
  // took the (b % 8)-th strip of consecutive element ids: 2268 against 2224 us of sub-cycle per
  // step, profiles/r05z)
  std::vector<int> bnd, inr, perm(E);
  for (int el = 0; el < E; el++) {
    bool b = false;
    for (int lf = 0; lf < 4; lf++) b = b || ebc[4 * el + lf] < 0;
    (b ? bnd : inr).push_back(el);
  }
  size_t ib = 0, ii = 0;
  // (measured, not kept: a CU's blocks on consecutive element ids -- neighbours sharing a CU --
  // 2357 against 2208 us of sub-cycle per step, profiles/r05ac)
  for (int b = 0; b < E; b++) {
    const bool light = (b % ncu) >= nheavy;
    perm[b] = (light && ib < bnd.size()) ? bnd[ib++] : (ii < inr.size() ? inr[ii++] : bnd[ib++]);
  }
  return perm;
}

}  // namespace hnumo
