// observers.hip -- what runs after a successful step of the resident state: the online flow
// statistics (kernels_stats.hip), the vorticity products (kernels_vort.hip), the eddy covariances
// (kernels_cov.hip), the energy budget (kernels_energy.hip, energy_plan.h), the region sets
// (kernels_region.hip, region_plan.h), the sample sets (kernels_sample.hip, sample_plan.h) and the float
// sets (kernels_float.hip, float_plan.h).
//
// Part of engine.hip's translation unit: included there once fail, HIPCHK and struct hnumo_engine
// (with Series and TreeSum) are defined.  All of it is plain launches on the engine stream outside
// the captured step: the step's launches, graph and bits are the same with or without observers.
//
// An observer writes: its kernel; its state in hnumo_engine with a Series (capacity 0 where it keeps none:
// `every` then stands alone and counts in series.steps all the same); X_free, called by hnumo_engine_destroy
// too; a begin that refuses its own arguments, then drain_and_free, its allocations (alloc_doubles,
// upload_optional, tree_alloc, series_begin) or begin_failed; an end through observer_end; a sample that
// launches on the engine stream; an arm of observers_after_step on series_due.  It gets from the pieces
// below: the refusals of its entry points with their texts and their precedence (no_engine, not_begun,
// null_arg, wrong_n, no_samples, no_state; set_by_id for the sets), the ring and its read (series_*), the
// tree sum, the paired sums' two layouts (sums_read, sums_write), the fields of such sums (fields_of_sums)
// and, from observer_layout.h, the index work of those and the launch grids, which run on the CPU too.
#include "observer_layout.h"

// ------------------------------------------------------------------ shared pieces
// ---- the way in.  Each states one refusal and is true when it refuses, with the message set.  An entry
// chains those that apply with || and returns HNUMO_ERR_INVALID; the order in the chain is which one wins --
// not begun, a NULL argument, a wrong n, no samples -- and the chain stands ahead of the entry's first HIP
// call wherever no refusal depends on the device (a broken device does not mask an argument error)
static bool no_engine(const hnumo_engine *eng) { return !eng; }

static bool refused(hnumo_engine *eng, const char *who, const std::string &why) {
  return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": " + why) != 0;
}

static bool not_begun(hnumo_engine *eng, bool on, const char *who, const char *begin) {
  return !on && refused(eng, who, std::string("call ") + begin + " first");
}

static bool null_arg(hnumo_engine *eng, const void *p, const char *who, const char *name) {
  return !p && refused(eng, who, std::string(name) + " is NULL");
}

// `shape`: what `name` counts, in the caller's words
static bool wrong_n(hnumo_engine *eng, int64_t n, int64_t want, const char *who, const char *shape, const char *name = "n") {
  return n != want && refused(eng, who, std::string(name) + " must be " + shape + " = " + std::to_string(want) + ", got " + std::to_string(n));
}

static bool wrong_M(hnumo_engine *eng, int64_t M, int64_t want, const char *who) {
  return M != want && refused(eng, who, "M must be the set's " + std::to_string(want) + ", got " + std::to_string(M));
}

// a begin's two counts, `names` in the caller's words
static bool negative(hnumo_engine *eng, int a, int b, const char *who, const char *names) {
  return (a < 0 || b < 0) && refused(eng, who, std::string(names) + " must be >= 0, got " + std::to_string(a) + ", " + std::to_string(b));
}

static bool no_samples(hnumo_engine *eng, int64_t nsamples, const char *who) { return nsamples == 0 && refused(eng, who, "no samples yet"); }

static bool no_state(hnumo_engine *eng, const char *who) {
  return !eng->has_state && refused(eng, who, "no state on the device yet (run a step first)");
}

// eng->L and eng->ngl as compile-time constants for a generic lambda (unsupported values are
// refused before any launch; the default arms are never taken for them)
template <class F>
static void with_L(int L, F &&f) {
  switch (L) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 3>{}); break;
  }
}

template <class F>
static void with_ngl(int ngl, F &&f) {
  switch (ngl) {
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

static bool sample_ngl_ok(int ngl) { return ngl == 3 || ngl == 4 || ngl == 5 || ngl == 6 || ngl == 8; }

// a copy back on the engine stream, waited for
static int download(hnumo_engine *eng, void *host, const void *dev, size_t bytes) {
  HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, eng->stream));
  HIPCHK(hipStreamSynchronize(eng->stream));
  HIPCHK(hipGetLastError());
  return HNUMO_OK;
}

static bool alloc_doubles(double **p, size_t n) { return hipMalloc((void **)p, (n ? n : 1) * sizeof(double)) == hipSuccess; }

// free these and null them
template <class... T>
static void dfree(T *&...p) {
  ((p ? (void)hipFree(p) : (void)0, p = nullptr), ...);
}

// the engine's device current and its stream drained: ahead of freeing or rewriting what a launch in flight uses
static int drain(hnumo_engine *eng) {
  HIPCHK(hipSetDevice(eng->device));
  HIPCHK(hipStreamSynchronize(eng->stream));
  return HNUMO_OK;
}

// ---- begin and end of a field observer, whose X_free frees its buffers and resets its state
// what a begin and an end start with (a sample in flight uses the old buffers)
static int drain_and_free(hnumo_engine *eng, void (*free_state)(hnumo_engine *)) {
  if (int rc = drain(eng)) return rc;
  free_state(eng);
  return HNUMO_OK;
}

// a copy of the caller's optional host[n] on the device (NULL: none, *d stays NULL); false: it failed
static bool upload_optional(double **d, const double *host, size_t n) {
  return !host || (alloc_doubles(d, n) && hipMemcpy(*d, host, n * sizeof(double), hipMemcpyHostToDevice) == hipSuccess);
}

// a begin whose allocations or uploads failed: nothing of it is left
static int begin_failed(hnumo_engine *eng, void (*free_state)(hnumo_engine *), const char *msg) {
  (void)hipGetLastError();
  free_state(eng);
  return fail(eng, HNUMO_ERR_DEVICE, msg);
}

// hnumo_X_end: a no-op before hnumo_X_begin
static int observer_end(hnumo_engine *eng, bool on, void (*free_state)(hnumo_engine *)) {
  return on ? drain_and_free(eng, free_state) : HNUMO_OK;
}

// the set `id` of sets[], or nullptr with the message set (the sets' X_set wrappers answer nullptr for no
// engine too); the first unused slot of sets[], or -1
template <class Set, int N>
static Set *set_by_id(hnumo_engine *eng, Set (&sets)[N], int32_t id, const char *who, const char *kind) {
  if (id >= 0 && id < N && sets[id].used) return &sets[id];
  refused(eng, who, std::string("no ") + kind + " set with id " + std::to_string(id));
  return nullptr;
}

template <class Set, int N>
static int free_slot(const Set (&sets)[N]) {
  for (int i = 0; i < N; i++)
    if (!sets[i].used) return i;
  return -1;
}

// ---- Series: a ring of `cap` entries of `width` doubles on the device.  every > 0: an entry is due
// after every every-th of the events counted in steps (successful steps; a float set's advances)
static void series_free(Series &s) {
  dfree(s.d);
  s = Series{};
}

// from empty again (the caller has drained the stream: a recording in flight writes the old ring)
static hipError_t series_begin(hnumo_engine *eng, Series &s, size_t width, int every, int cap, bool zero) {
  series_free(s);
  s.width = width;
  if (cap > 0) {
    hipError_t err = hipMalloc((void **)&s.d, (size_t)cap * width * sizeof(double));
    if (err == hipSuccess && zero) err = hipMemsetAsync(s.d, 0, (size_t)cap * width * sizeof(double), eng->stream);
    if (err != hipSuccess) {
      (void)hipGetLastError();
      series_free(s);
      return err;
    }
  }
  s.every = every;
  s.cap = cap;
  return hipSuccess;
}

static bool series_due(Series &s) { return s.every > 0 && ++s.steps % s.every == 0; }

static double *series_slot(const Series &s) { return s.d + (size_t)s.count * s.width; }

// 0 while there is room, else the refusal: "<who>: <which> is full (<cap> <entries>): nothing <done>; ..."
static int series_full(hnumo_engine *eng, const Series &s, const char *who, const std::string &which, const char *entries,
                       const char *done) {
  if (s.count < s.cap) return 0;
  return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": " + which + " is full (" + std::to_string(s.cap) + " " + entries +
                                          "): nothing " + done + "; read it with clear = 1");
}

// the entries held into `out` (NULL: the count alone), as they are (V = 0) or each from planar [V][M]
// to (V,M); `shape`: the entry's width in the caller's words
static int series_read(hnumo_engine *eng, Series &s, int V, size_t M, double *out, int64_t n, int64_t *count, int32_t clear,
                       const char *who, const char *shape) {
  const int64_t want = (int64_t)s.width * s.count;
  if (n < 0 || (out && n < want))
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": out holds n = " + std::to_string(n) +
                                            " values, the series has " + shape + "*count = " + std::to_string(want));
  HIPCHK(hipSetDevice(eng->device));
  if (out && want > 0) {
    std::vector<double> raw(V ? (size_t)want : 0);
    if (int rc = download(eng, V ? raw.data() : out, s.d, (size_t)want * sizeof(double))) return rc;
    if (V) sample_transpose(raw.data(), V, M, (size_t)s.count, out);
  }
  if (count) *count = s.count;
  // (the next entry's slot is written after this copy on the same stream)
  if (clear && out) s.count = 0;
  return HNUMO_OK;
}

// ---- TreeSum: `rows` rows of per-element partials [rows][ne] summed pairwise over aligned chunks,
// the same tree for any ne (kernels_stats.hip: stats_tree_kernel)
static bool tree_alloc(TreeSum &t, int rows, int ne) {
  const size_t nch = ((size_t)ne + ST_CHUNK - 1) / ST_CHUNK;
  return alloc_doubles(&t.part, (size_t)rows * ne) && alloc_doubles(&t.tree[0], rows * nch) &&
         alloc_doubles(&t.tree[1], rows * ((nch + ST_CHUNK - 1) / ST_CHUNK));
}

static void tree_free(TreeSum &t) { dfree(t.part, t.tree[0], t.tree[1]); }

// passes over aligned chunks until one value per row is left, which the last pass writes to dst[rows]
static void tree_sum(hnumo_engine *eng, const TreeSum &t, int rows, int ne, double *dst) {
  const double *in = t.part;
  int n = ne, pass = 0;
  for (;;) {
    const int nch = (n + ST_CHUNK - 1) / ST_CHUNK;
    const bool last = nch == 1;
    double *out = last ? dst : t.tree[pass & 1];
    hipLaunchKernelGGL(stats_tree_kernel, dim3(nch, rows), dim3(ST_BS), 0, eng->stream, in, n, out, last ? 1 : nch);
    if (last) break;
    in = out;
    n = nch;
    pass++;
  }
}

// ---- paired running sums (statistics: NP = 2, covariances: NP = CV_NPAIR) between the device's
// [L][NP][npoin][2] and the caller's (2*NP,npoin,L); `shape`: that size in the caller's words
static int sums_read(hnumo_engine *eng, bool on, const double *sums, int NP, double *out, int64_t n, const char *who,
                     const char *begin, const char *shape) {
  const size_t want = 2 * (size_t)NP * eng->npoin * eng->L;
  if (not_begun(eng, on, who, begin) || null_arg(eng, out, who, "out") || wrong_n(eng, n, (int64_t)want, who, shape))
    return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  std::vector<double> raw(want);
  if (int rc = download(eng, raw.data(), sums, want * sizeof(double))) return rc;
  pairs_unpack(raw.data(), NP, eng->L, (size_t)eng->npoin, out);
  return HNUMO_OK;
}

static int sums_write(hnumo_engine *eng, bool on, double *sums, int NP, const double *in, int64_t n, int64_t nsamples,
                      const char *who, const char *begin, const char *shape) {
  const size_t want = 2 * (size_t)NP * eng->npoin * eng->L;
  if (not_begun(eng, on, who, begin) || null_arg(eng, in, who, "in") || wrong_n(eng, n, (int64_t)want, who, shape) ||
      (nsamples < 0 && refused(eng, who, "nsamples must be >= 0")))
    return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  std::vector<double> raw(want);
  pairs_pack(in, NP, eng->L, (size_t)eng->npoin, raw.data());
  HIPCHK(hipMemcpyAsync(sums, raw.data(), want * sizeof(double), hipMemcpyHostToDevice, eng->stream));
  HIPCHK(hipStreamSynchronize(eng->stream));
  return HNUMO_OK;
}

// the fields derived from such sums, `want` doubles into `out`: scratch on the device, the observer's
// launch(workgroups of `bs` lanes over the nodes, npoin, owned nodes, scratch), the copy back
template <class Launch>
static int fields_of_sums(hnumo_engine *eng, int64_t want, int bs, double *out, Launch &&launch) {
  HIPCHK(hipSetDevice(eng->device));
  double *d = nullptr;
  HIPCHK(hipMalloc((void **)&d, (size_t)want * sizeof(double)));
  const size_t npoin = (size_t)eng->npoin;
  launch(block_count(npoin, bs, 4096), npoin, (size_t)eng->nelem_owned * eng->P, d);
  const int rc = download(eng, out, d, (size_t)want * sizeof(double));
  (void)hipFree(d);
  return rc;
}

// ------------------------------------------------------------------ online flow statistics
// eng->stats: the running sums [L][2][npoin] pairs, the element partials [2L][ne] and their tree, the
// series [capacity][L][2]; nsamples: samples taken since begin
static void stats_free(hnumo_engine *eng) {
  auto &st = eng->stats;
  dfree(st.sums);
  tree_free(st.tree);
  series_free(st.series);
  st.on = false;
  st.nsamples = 0;
}

static size_t stats_nsums(const hnumo_engine *eng) { return 4 * (size_t)eng->npoin * eng->L; }

extern "C" int hnumo_stats_begin(hnumo_engine *eng, int32_t every, int32_t series_capacity) {
  const char *who = "hnumo_stats_begin";
  if (no_engine(eng) || negative(eng, every, series_capacity, who, "every and series_capacity")) return HNUMO_ERR_INVALID;
  if (eng->L < 1 || eng->L > MAXL || eng->ngl < 2 || eng->ngl * eng->ngl > ST_BS)
    return fail(eng, HNUMO_ERR_INVALID, "hnumo_stats_begin: unsupported nlayers or ngl");
  if (int rc = drain_and_free(eng, stats_free)) return rc;
  auto &st = eng->stats;
  const int rows = 2 * eng->L;
  if (!alloc_doubles(&st.sums, stats_nsums(eng)) || (series_capacity > 0 && !tree_alloc(st.tree, rows, eng->nelem_owned)) ||
      series_begin(eng, st.series, rows, every, series_capacity, true) != hipSuccess)
    return begin_failed(eng, stats_free, "hnumo_stats_begin: device allocation failed");
  HIPCHK(hipMemsetAsync(st.sums, 0, stats_nsums(eng) * sizeof(double), eng->stream));
  st.on = true;
  return HNUMO_OK;
}

extern "C" int hnumo_stats_end(hnumo_engine *eng) {
  return no_engine(eng) ? HNUMO_ERR_INVALID : observer_end(eng, eng->stats.on, stats_free);
}

// one sample of the state on the device, ordered after what is on the engine stream; no copy back
static int stats_sample(hnumo_engine *eng, const char *who) {
  auto &st = eng->stats;
  if (not_begun(eng, st.on, who, "hnumo_stats_begin") || no_state(eng, who)) return HNUMO_ERR_INVALID;
  const bool series = st.series.cap > 0;
  if (series)
    if (int rc = series_full(eng, st.series, who, "the series", "samples", "accumulated")) return rc;
  const int ne = eng->nelem_owned, EPB = ST_BS / eng->P;
  if (ne > 0) {
    StatsArgs a{};
    a.q = eng->q;
    a.alpha = eng->alpha;
    a.w = eng->nstat + (size_t)NS_W * eng->npoin;
    a.sums = (double2 *)st.sums;
    a.part = st.tree.part;
    a.gravity = eng->p.gravity;
    a.npoin = eng->npoin;
    a.ne = ne;
    a.ngl = eng->ngl;
    const int nb = block_count(ne, EPB);
    with_L(eng->L, [&](auto l) {
      constexpr int L = decltype(l)::value;
      if (series)
        hipLaunchKernelGGL((stats_accumulate_kernel<L, true>), dim3(nb), dim3(ST_BS), 0, eng->stream, a);
      else
        hipLaunchKernelGGL((stats_accumulate_kernel<L, false>), dim3(nb), dim3(ST_BS), 0, eng->stream, a);
    });
    if (series) tree_sum(eng, st.tree, 2 * eng->L, ne, series_slot(st.series));
    HIPCHK(hipGetLastError());
  }
  if (series) st.series.count++;
  st.nsamples++;
  return HNUMO_OK;
}

extern "C" int hnumo_stats_accumulate(hnumo_engine *eng) {
  if (no_engine(eng)) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  return stats_sample(eng, "hnumo_stats_accumulate");
}

extern "C" int hnumo_stats_sums(hnumo_engine *eng, double *out, int64_t n, int64_t *nsamples) {
  if (no_engine(eng)) return HNUMO_ERR_INVALID;
  const auto &st = eng->stats;
  if (int rc = sums_read(eng, st.on, st.sums, 2, out, n, "hnumo_stats_sums", "hnumo_stats_begin", "4*npoin*nlayers")) return rc;
  if (nsamples) *nsamples = st.nsamples;
  return HNUMO_OK;
}

extern "C" int hnumo_stats_set_sums(hnumo_engine *eng, const double *in, int64_t n, int64_t nsamples) {
  if (no_engine(eng)) return HNUMO_ERR_INVALID;
  auto &st = eng->stats;
  if (int rc = sums_write(eng, st.on, st.sums, 2, in, n, nsamples, "hnumo_stats_set_sums", "hnumo_stats_begin", "4*npoin*nlayers"))
    return rc;
  st.nsamples = nsamples;
  return HNUMO_OK;
}

extern "C" int hnumo_stats_fields(hnumo_engine *eng, double *out, int64_t n) {
  const char *who = "hnumo_stats_fields";
  if (no_engine(eng)) return HNUMO_ERR_INVALID;
  const auto &st = eng->stats;
  const int64_t want = 5 * (int64_t)eng->npoin * eng->L;
  if (not_begun(eng, st.on, who, "hnumo_stats_begin") || null_arg(eng, out, who, "out") ||
      wrong_n(eng, n, want, who, "5*npoin*nlayers") || no_samples(eng, st.nsamples, who))
    return HNUMO_ERR_INVALID;
  return fields_of_sums(eng, want, ST_BS, out, [&](int nb, size_t npoin, size_t nown, double *d) {
    with_L(eng->L, [&](auto l) {
      hipLaunchKernelGGL(stats_fields_kernel<decltype(l)::value>, dim3(nb), dim3(ST_BS), 0, eng->stream, (const double2 *)st.sums,
                         npoin, nown, (double)st.nsamples, d);
    });
  });
}

extern "C" int hnumo_stats_series(hnumo_engine *eng, double *out, int64_t n, int64_t *count, int32_t clear) {
  const char *who = "hnumo_stats_series";
  if (no_engine(eng) || not_begun(eng, eng->stats.on, who, "hnumo_stats_begin")) return HNUMO_ERR_INVALID;
  return series_read(eng, eng->stats.series, 0, 0, out, n, count, clear, who, "2*nlayers");
}

// ------------------------------------------------------------------ vorticity products
// eng->vort: the caller's coriolis_df (NULL: f = 0), the fields of the last sample planar
// [L][4][npoin], the element partials [3L][ne] and their tree, the series [capacity][L][3]
static void vort_free(hnumo_engine *eng) {
  auto &vt = eng->vort;
  dfree(vt.f, vt.fields);
  tree_free(vt.tree);
  series_free(vt.series);
  vt.on = false;
}

static size_t vort_nfields(const hnumo_engine *eng) { return 4 * (size_t)eng->npoin * eng->L; }

extern "C" int hnumo_vort_begin(hnumo_engine *eng, const double *coriolis_df, int32_t every, int32_t series_capacity) {
  const char *who = "hnumo_vort_begin";
  if (no_engine(eng) || negative(eng, every, series_capacity, who, "every and series_capacity")) return HNUMO_ERR_INVALID;
  if (eng->L < 1 || eng->L > MAXL || !sample_ngl_ok(eng->ngl))
    return fail(eng, HNUMO_ERR_INVALID, "hnumo_vort_begin: unsupported nlayers or ngl");
  if (int rc = drain_and_free(eng, vort_free)) return rc;
  auto &vt = eng->vort;
  const int rows = 3 * eng->L;
  if (!alloc_doubles(&vt.fields, vort_nfields(eng)) || !upload_optional(&vt.f, coriolis_df, (size_t)eng->npoin) ||
      (series_capacity > 0 && !tree_alloc(vt.tree, rows, eng->nelem_owned)) ||
      series_begin(eng, vt.series, rows, every, series_capacity, true) != hipSuccess)
    return begin_failed(eng, vort_free, "hnumo_vort_begin: device allocation or upload failed");
  // (the nodes of ghost elements are never written: they read 0)
  HIPCHK(hipMemsetAsync(vt.fields, 0, vort_nfields(eng) * sizeof(double), eng->stream));
  vt.on = true;
  return HNUMO_OK;
}

extern "C" int hnumo_vort_end(hnumo_engine *eng) {
  return no_engine(eng) ? HNUMO_ERR_INVALID : observer_end(eng, eng->vort.on, vort_free);
}

// the fields of the state on the device into vort.fields, with `series` the next series entry too;
// ordered after what is on the engine stream, no copy back
static int vort_form(hnumo_engine *eng, bool series, const char *who) {
  auto &vt = eng->vort;
  if (not_begun(eng, vt.on, who, "hnumo_vort_begin") || no_state(eng, who) ||
      (series && vt.series.cap == 0 && refused(eng, who, "no series (hnumo_vort_begin with series_capacity = 0)")))
    return HNUMO_ERR_INVALID;
  if (series)
    if (int rc = series_full(eng, vt.series, who, "the series", "samples", "recorded")) return rc;
  const int ne = eng->nelem_owned, EPB = VT_BS / eng->P;
  if (ne > 0) {
    VortArgs a{};
    a.q = eng->q;
    a.alpha = eng->alpha;
    a.nstat = eng->nstat;
    a.f = vt.f;
    a.dpsi = eng->basis + 2 * (size_t)eng->ngl * eng->nq;
    a.out = vt.fields;
    a.part = vt.tree.part;
    a.gravity = eng->p.gravity;
    a.npoin = eng->npoin;
    a.ne = ne;
    const int nb = block_count(ne, EPB);
    with_ngl(eng->ngl, [&](auto ngl) {
      with_L(eng->L, [&](auto l) {
        constexpr int NGL = decltype(ngl)::value, L = decltype(l)::value;
        if (series)
          hipLaunchKernelGGL((vort_kernel<NGL, L, true>), dim3(nb), dim3(VT_BS), 0, eng->stream, a);
        else
          hipLaunchKernelGGL((vort_kernel<NGL, L, false>), dim3(nb), dim3(VT_BS), 0, eng->stream, a);
      });
    });
    if (series) tree_sum(eng, vt.tree, 3 * eng->L, ne, series_slot(vt.series));
    HIPCHK(hipGetLastError());
  }
  if (series) vt.series.count++;
  return HNUMO_OK;
}

extern "C" int hnumo_vort_record(hnumo_engine *eng) {
  if (no_engine(eng)) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  return vort_form(eng, true, "hnumo_vort_record");
}

extern "C" int hnumo_vort_fields(hnumo_engine *eng, double *out, int64_t n) {
  const char *who = "hnumo_vort_fields";
  if (no_engine(eng) || not_begun(eng, eng->vort.on, who, "hnumo_vort_begin") || null_arg(eng, out, who, "out") ||
      wrong_n(eng, n, (int64_t)vort_nfields(eng), who, "4*npoin*nlayers"))
    return HNUMO_ERR_INVALID;
  const size_t want = vort_nfields(eng), npoin = (size_t)eng->npoin;
  HIPCHK(hipSetDevice(eng->device));
  if (int rc = vort_form(eng, false, who)) return rc;
  std::vector<double> raw(want);
  if (int rc = download(eng, raw.data(), eng->vort.fields, want * sizeof(double))) return rc;
  // planar [L][4][npoin] -> the caller's (4,npoin,L)
  for (int k = 0; k < eng->L; k++) sample_transpose(raw.data() + 4 * npoin * k, 4, npoin, 1, out + 4 * npoin * k);
  return HNUMO_OK;
}

extern "C" int hnumo_vort_series(hnumo_engine *eng, double *out, int64_t n, int64_t *count, int32_t clear) {
  const char *who = "hnumo_vort_series";
  if (no_engine(eng) || not_begun(eng, eng->vort.on, who, "hnumo_vort_begin")) return HNUMO_ERR_INVALID;
  return series_read(eng, eng->vort.series, 0, 0, out, n, count, clear, who, "3*nlayers");
}

// ------------------------------------------------------------------ eddy covariances
// eng->cov: the caller's coriolis_df and zref (NULL: 0), the running sums [L][7][npoin] pairs, the
// element partials [3L][ne] of the integrals with their tree and the integrals [3L]; nsamples: samples
// taken since begin.  The series has capacity 0: its every and steps alone say when a sample is due
static void cov_free(hnumo_engine *eng) {
  auto &cv = eng->cov;
  dfree(cv.f, cv.zref, cv.sums, cv.integ);
  tree_free(cv.tree);
  series_free(cv.series);
  cv.on = false;
  cv.nsamples = 0;
}

static size_t cov_nsums(const hnumo_engine *eng) { return CV_NSUM * (size_t)eng->npoin * eng->L; }

// L = 2 or 3 as a compile-time constant (hnumo_cov_begin refuses the rest)
template <class F>
static void cov_with_L(int L, F &&f) {
  if (L == 2)
    f(std::integral_constant<int, 2>{});
  else
    f(std::integral_constant<int, 3>{});
}

extern "C" int hnumo_cov_begin(hnumo_engine *eng, const double *coriolis_df, const double *zref, int32_t every) {
  if (no_engine(eng)) return HNUMO_ERR_INVALID;
  if (every < 0) return fail(eng, HNUMO_ERR_INVALID, "hnumo_cov_begin: every must be >= 0, got " + std::to_string(every));
  if (eng->L < 2 || eng->L > MAXL || !sample_ngl_ok(eng->ngl))
    return fail(eng, HNUMO_ERR_INVALID, "hnumo_cov_begin: unsupported nlayers or ngl (nlayers 2 or 3; ngl 3, 4, 5, 6 or 8), got " +
                                            std::to_string(eng->L) + ", " + std::to_string(eng->ngl));
  if (int rc = drain_and_free(eng, cov_free)) return rc;
  auto &cv = eng->cov;
  const size_t npoin = (size_t)eng->npoin;
  const int rows = CV_NINT * eng->L;
  // (the tree serves hnumo_cov_integrals, whatever `every`; capacity 0 allocates no ring)
  if (!alloc_doubles(&cv.sums, cov_nsums(eng)) || !alloc_doubles(&cv.integ, (size_t)rows) ||
      !tree_alloc(cv.tree, rows, eng->nelem_owned) || !upload_optional(&cv.f, coriolis_df, npoin) ||
      !upload_optional(&cv.zref, zref, npoin * eng->L) || series_begin(eng, cv.series, rows, every, 0, false) != hipSuccess)
    return begin_failed(eng, cov_free, "hnumo_cov_begin: device allocation or upload failed");
  // (the nodes of ghost elements are never accumulated: their sums stay +0.0)
  HIPCHK(hipMemsetAsync(cv.sums, 0, cov_nsums(eng) * sizeof(double), eng->stream));
  cv.on = true;
  return HNUMO_OK;
}

extern "C" int hnumo_cov_end(hnumo_engine *eng) {
  return no_engine(eng) ? HNUMO_ERR_INVALID : observer_end(eng, eng->cov.on, cov_free);
}

static CovArgs cov_args(hnumo_engine *eng) {
  auto &cv = eng->cov;
  CovArgs a{};
  a.q = eng->q;
  a.alpha = eng->alpha;
  a.nstat = eng->nstat;
  a.f = cv.f;
  a.zref = cv.zref;
  a.dpsi = eng->basis + 2 * (size_t)eng->ngl * eng->nq;
  a.sums = (double2 *)cv.sums;
  a.part = cv.tree.part;
  a.gravity = eng->p.gravity;
  a.nsamp = (double)cv.nsamples;
  a.npoin = eng->npoin;
  a.ne = eng->nelem_owned;
  a.ngl = eng->ngl;
  return a;
}

// one sample of the state on the device, ordered after what is on the engine stream; no copy back
static int cov_sample(hnumo_engine *eng, const char *who) {
  auto &cv = eng->cov;
  if (not_begun(eng, cv.on, who, "hnumo_cov_begin") || no_state(eng, who)) return HNUMO_ERR_INVALID;
  const int ne = eng->nelem_owned, EPB = CV_BS / eng->P;
  if (ne > 0) {
    const CovArgs a = cov_args(eng);
    const int nb = block_count(ne, EPB);
    with_ngl(eng->ngl, [&](auto ngl) {
      cov_with_L(eng->L, [&](auto l) {
        constexpr int NGL = decltype(ngl)::value, L = decltype(l)::value;
        hipLaunchKernelGGL((cov_accumulate_kernel<NGL, L>), dim3(nb), dim3(CV_BS), 0, eng->stream, a);
      });
    });
    HIPCHK(hipGetLastError());
  }
  cv.nsamples++;
  return HNUMO_OK;
}

extern "C" int hnumo_cov_accumulate(hnumo_engine *eng) {
  if (no_engine(eng)) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  return cov_sample(eng, "hnumo_cov_accumulate");
}

static_assert(CV_NSUM == 2 * CV_NPAIR, "the caller's (14,npoin,L) is the pairs' two halves side by side");

extern "C" int hnumo_cov_sums(hnumo_engine *eng, double *out, int64_t n, int64_t *nsamples) {
  if (no_engine(eng)) return HNUMO_ERR_INVALID;
  const auto &cv = eng->cov;
  if (int rc = sums_read(eng, cv.on, cv.sums, CV_NPAIR, out, n, "hnumo_cov_sums", "hnumo_cov_begin", "14*npoin*nlayers")) return rc;
  if (nsamples) *nsamples = cv.nsamples;
  return HNUMO_OK;
}

extern "C" int hnumo_cov_set_sums(hnumo_engine *eng, const double *in, int64_t n, int64_t nsamples) {
  if (no_engine(eng)) return HNUMO_ERR_INVALID;
  auto &cv = eng->cov;
  if (int rc = sums_write(eng, cv.on, cv.sums, CV_NPAIR, in, n, nsamples, "hnumo_cov_set_sums", "hnumo_cov_begin", "14*npoin*nlayers"))
    return rc;
  cv.nsamples = nsamples;
  return HNUMO_OK;
}

extern "C" int hnumo_cov_fields(hnumo_engine *eng, double *out, int64_t n) {
  const char *who = "hnumo_cov_fields";
  if (no_engine(eng)) return HNUMO_ERR_INVALID;
  const auto &cv = eng->cov;
  const int64_t want = CV_NFIELD * (int64_t)eng->npoin * eng->L;
  if (not_begun(eng, cv.on, who, "hnumo_cov_begin") || null_arg(eng, out, who, "out") ||
      wrong_n(eng, n, want, who, "16*npoin*nlayers") || no_samples(eng, cv.nsamples, who))
    return HNUMO_ERR_INVALID;
  return fields_of_sums(eng, want, CV_BS, out, [&](int nb, size_t npoin, size_t nown, double *d) {
    cov_with_L(eng->L, [&](auto l) {
      hipLaunchKernelGGL(cov_fields_kernel<decltype(l)::value>, dim3(nb), dim3(CV_BS), 0, eng->stream, (const double2 *)cv.sums,
                         npoin, nown, (double)cv.nsamples, d);
    });
  });
}

// out(3,nlayers): the element partials, then the tree of the statistics' series
extern "C" int hnumo_cov_integrals(hnumo_engine *eng, double *out, int64_t n) {
  const char *who = "hnumo_cov_integrals";
  if (no_engine(eng)) return HNUMO_ERR_INVALID;
  const int rows = CV_NINT * eng->L;
  if (not_begun(eng, eng->cov.on, who, "hnumo_cov_begin") || null_arg(eng, out, who, "out") ||
      wrong_n(eng, n, rows, who, "3*nlayers") || no_samples(eng, eng->cov.nsamples, who))
    return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  const int ne = eng->nelem_owned, EPB = CV_BS / eng->P;
  if (ne == 0) {
    for (int r = 0; r < rows; r++) out[r] = 0.0;
    return HNUMO_OK;
  }
  const CovArgs a = cov_args(eng);
  const int nb = block_count(ne, EPB);
  cov_with_L(eng->L, [&](auto l) {
    hipLaunchKernelGGL(cov_integrals_kernel<decltype(l)::value>, dim3(nb), dim3(CV_BS), 0, eng->stream, a);
  });
  tree_sum(eng, eng->cov.tree, rows, ne, eng->cov.integ);
  HIPCHK(hipGetLastError());
  return download(eng, out, eng->cov.integ, (size_t)rows * sizeof(double));
}

// ------------------------------------------------------------------ energy budget
// eng->energy: the caller's zref (NULL: 0), the running sums (S_W, S_D) [npoin_q] pairs and S_V
// [L][npoin], the element partials [3L+2][ne] and their tree, the series [capacity][3L+2]; nsamples:
// samples taken since begin
static void energy_free(hnumo_engine *eng) {
  auto &en = eng->energy;
  dfree(en.zref, en.sq, en.sv);
  tree_free(en.tree);
  series_free(en.series);
  en.on = false;
  en.nsamples = 0;
}

static size_t energy_nquad(const hnumo_engine *eng) { return 2 * (size_t)eng->npq; }
static size_t energy_nnodal(const hnumo_engine *eng) { return (size_t)eng->npoin * eng->L; }

extern "C" int hnumo_energy_begin(hnumo_engine *eng, const double *zref, int32_t every, int32_t series_capacity) {
  const char *who = "hnumo_energy_begin";
  if (no_engine(eng) || negative(eng, every, series_capacity, who, "every and series_capacity")) return HNUMO_ERR_INVALID;
  if (eng->L < 1 || eng->L > MAXL || !sample_ngl_ok(eng->ngl) || eng->nq != 2 * eng->ngl - 1)
    return fail(eng, HNUMO_ERR_INVALID, "hnumo_energy_begin: unsupported nlayers or ngl (nlayers 1..3; ngl 3, 4, 5, 6 or 8), got " +
                                            std::to_string(eng->L) + ", " + std::to_string(eng->ngl));
  if (int rc = drain_and_free(eng, energy_free)) return rc;
  auto &en = eng->energy;
  const int rows = en_rows(eng->L);
  if (!alloc_doubles(&en.sq, energy_nquad(eng)) || !alloc_doubles(&en.sv, energy_nnodal(eng)) ||
      (series_capacity > 0 && !tree_alloc(en.tree, rows, eng->nelem_owned)) || !upload_optional(&en.zref, zref, energy_nnodal(eng)) ||
      series_begin(eng, en.series, rows, every, series_capacity, true) != hipSuccess)
    return begin_failed(eng, energy_free, "hnumo_energy_begin: device allocation or upload failed");
  // (the points of ghost elements are never visited: their sums stay +0.0)
  HIPCHK(hipMemsetAsync(en.sq, 0, energy_nquad(eng) * sizeof(double), eng->stream));
  HIPCHK(hipMemsetAsync(en.sv, 0, energy_nnodal(eng) * sizeof(double), eng->stream));
  en.on = true;
  return HNUMO_OK;
}

extern "C" int hnumo_energy_end(hnumo_engine *eng) {
  return no_engine(eng) ? HNUMO_ERR_INVALID : observer_end(eng, eng->energy.on, energy_free);
}

template <int NGL, int L, bool SERIES>
static void energy_launch(int botfr, int nb, hipStream_t st, const EnergyArgs &a) {
  switch (botfr) {
    case 0: hipLaunchKernelGGL((energy_sample_kernel<NGL, L, 0, SERIES>), dim3(nb), dim3(EN_BS), 0, st, a); break;
    case 1: hipLaunchKernelGGL((energy_sample_kernel<NGL, L, 1, SERIES>), dim3(nb), dim3(EN_BS), 0, st, a); break;
    default: hipLaunchKernelGGL((energy_sample_kernel<NGL, L, 2, SERIES>), dim3(nb), dim3(EN_BS), 0, st, a); break;
  }
}

// one sample of the state and the wind on the device, ordered after what is on the engine stream; no
// copy back
static int energy_sample(hnumo_engine *eng, const char *who) {
  auto &en = eng->energy;
  if (not_begun(eng, en.on, who, "hnumo_energy_begin") || no_state(eng, who) ||
      ((eng->p.botfr < 0 || eng->p.botfr > 2) && refused(eng, who, "botfr must be 0, 1 or 2, got " + std::to_string(eng->p.botfr))))
    return HNUMO_ERR_INVALID;
  const bool series = en.series.cap > 0;
  if (series)
    if (int rc = series_full(eng, en.series, who, "the series", "samples", "accumulated")) return rc;
  const int ne = eng->nelem_owned, EPG = en_epg(eng->ngl);
  if (ne > 0) {
    EnergyArgs a{};
    a.q = eng->q;
    a.alpha = eng->alpha;
    a.nstat = eng->nstat;
    a.qstat = eng->qstat;
    a.zref = en.zref;
    a.psiq = eng->basis;
    a.dpsi = eng->basis + 2 * (size_t)eng->ngl * eng->nq;
    a.sq = (double2 *)en.sq;
    a.sv = en.sv;
    a.part = en.tree.part;
    a.gravity = eng->p.gravity;
    a.cd = eng->p.cd_mlswe;
    a.visc = eng->p.visc_mlswe;
    a.npoin = eng->npoin;
    a.npq = eng->npq;
    a.ne = ne;
    const int nb = block_count(ne, EPG);
    with_ngl(eng->ngl, [&](auto ngl) {
      with_L(eng->L, [&](auto l) {
        constexpr int NGL = decltype(ngl)::value, L = decltype(l)::value;
        if (series)
          energy_launch<NGL, L, true>(eng->p.botfr, nb, eng->stream, a);
        else
          energy_launch<NGL, L, false>(eng->p.botfr, nb, eng->stream, a);
      });
    });
    if (series) tree_sum(eng, en.tree, en_rows(eng->L), ne, series_slot(en.series));
    HIPCHK(hipGetLastError());
  }
  if (series) en.series.count++;
  en.nsamples++;
  return HNUMO_OK;
}

extern "C" int hnumo_energy_sample(hnumo_engine *eng) {
  if (no_engine(eng)) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  return energy_sample(eng, "hnumo_energy_sample");
}

extern "C" int hnumo_energy_series(hnumo_engine *eng, double *out, int64_t n, int64_t *count, int32_t clear) {
  const char *who = "hnumo_energy_series";
  if (no_engine(eng) || not_begun(eng, eng->energy.on, who, "hnumo_energy_begin") ||
      (eng->energy.series.cap == 0 && refused(eng, who, "no series (hnumo_energy_begin was given series_capacity = 0)")))
    return HNUMO_ERR_INVALID;
  return series_read(eng, eng->energy.series, 0, 0, out, n, count, clear, who, "(3*nlayers+2)");
}

// what hnumo_energy_sums, _set_sums and _means refuse alike: not begun, a NULL buffer, a wrong nq2 or nn
static bool energy_sums_refused(hnumo_engine *eng, const void *quad2, int64_t nq2, const void *nodal, int64_t nn, const char *who) {
  return no_engine(eng) || not_begun(eng, eng->energy.on, who, "hnumo_energy_begin") ||
         ((!quad2 || !nodal) && refused(eng, who, "quad2 or nodal is NULL")) ||
         wrong_n(eng, nq2, (int64_t)energy_nquad(eng), who, "2*npoin_q", "nq2") ||
         wrong_n(eng, nn, (int64_t)energy_nnodal(eng), who, "npoin*nlayers", "nn");
}

// (the device layouts are the caller's: (2,npoin_q) and (npoin,nlayers))
extern "C" int hnumo_energy_sums(hnumo_engine *eng, double *quad2, int64_t nq2, double *nodal, int64_t nn, int64_t *nsamples) {
  if (energy_sums_refused(eng, quad2, nq2, nodal, nn, "hnumo_energy_sums")) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  HIPCHK(hipMemcpyAsync(quad2, eng->energy.sq, (size_t)nq2 * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
  if (int rc = download(eng, nodal, eng->energy.sv, (size_t)nn * sizeof(double))) return rc;
  if (nsamples) *nsamples = eng->energy.nsamples;
  return HNUMO_OK;
}

extern "C" int hnumo_energy_set_sums(hnumo_engine *eng, const double *quad2, int64_t nq2, const double *nodal, int64_t nn,
                                     int64_t nsamples) {
  const char *who = "hnumo_energy_set_sums";
  if (energy_sums_refused(eng, quad2, nq2, nodal, nn, who) || (nsamples < 0 && refused(eng, who, "nsamples must be >= 0")))
    return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  HIPCHK(hipMemcpyAsync(eng->energy.sq, quad2, (size_t)nq2 * sizeof(double), hipMemcpyHostToDevice, eng->stream));
  HIPCHK(hipMemcpyAsync(eng->energy.sv, nodal, (size_t)nn * sizeof(double), hipMemcpyHostToDevice, eng->stream));
  HIPCHK(hipStreamSynchronize(eng->stream));
  eng->energy.nsamples = nsamples;
  return HNUMO_OK;
}

// the sums divided by double(nsamples), on the host: S_W/N, S_D/N (2,npoin_q) and S_V/N (npoin,nlayers)
extern "C" int hnumo_energy_means(hnumo_engine *eng, double *quad2, int64_t nq2, double *nodal, int64_t nn) {
  const char *who = "hnumo_energy_means";
  if (energy_sums_refused(eng, quad2, nq2, nodal, nn, who) || no_samples(eng, eng->energy.nsamples, who)) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  HIPCHK(hipMemcpyAsync(quad2, eng->energy.sq, (size_t)nq2 * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
  if (int rc = download(eng, nodal, eng->energy.sv, (size_t)nn * sizeof(double))) return rc;
  const double N = (double)eng->energy.nsamples;
  for (int64_t x = 0; x < nq2; x++) quad2[x] = quad2[x] / N;
  for (int64_t x = 0; x < nn; x++) nodal[x] = nodal[x] / N;
  return HNUMO_OK;
}

// ------------------------------------------------------------------ region sets
// eng->regions[]: the host plan (region_plan.h), the member list and the passes' descriptors on the device,
// the member partials [V][nmem] with the two level buffers, the areas and the series [capacity][V][R]
using RegionSet = hnumo_engine::RegionSet;

static void regions_flag(hnumo_engine *eng) {
  eng->regions_on = false;
  for (const auto &s : eng->regions) eng->regions_on = eng->regions_on || (s.used && s.series.every > 0);
}

static void regions_free(hnumo_engine *eng, int id) {
  auto &s = eng->regions[id];
  dfree(s.f, s.part, s.lvl[0], s.lvl[1]);
  dfree(s.d_mem);
  dfree(s.d_desc);
  series_free(s.series);
  s = RegionSet{};
  regions_flag(eng);
}

static RegionSet *regions_set(hnumo_engine *eng, int32_t id, const char *who) {
  return no_engine(eng) ? nullptr : set_by_id(eng, eng->regions, id, who, "region");
}

static bool regions_no_series(hnumo_engine *eng, const RegionSet &s, int id, const char *who) {
  return s.series.cap == 0 && refused(eng, who, "region set " + std::to_string(id) +
                                                    " has no series (hnumo_regions_create was given series_capacity = 0)");
}

// the passes of the set's plan over `rows` rows of s.part into entry [rows][R]: one launch per pass,
// whatever the number of regions
static void regions_tree(hnumo_engine *eng, const RegionSet &s, int rows, double *entry) {
  const double *in = s.part;
  const RegionChunk *d = s.d_desc;
  for (size_t p = 0; p < s.plan.pass.size(); p++) {
    const RegionPass &ps = s.plan.pass[p];
    double *next = s.lvl[p & 1];
    hipLaunchKernelGGL(region_tree_kernel, dim3((unsigned)ps.chunks.size(), rows), dim3(RG_BS), 0, eng->stream, (const int4 *)d, in,
                       (size_t)ps.nin, next, (size_t)ps.nout, entry, s.plan.R);
    d += ps.chunks.size();
    in = next;
  }
}

extern "C" int hnumo_regions_create(hnumo_engine *eng, const int32_t *region_of_elem, int64_t n, int32_t nregions, int32_t rows_mask,
                                    const double *coriolis_df, int32_t every, int32_t series_capacity, int32_t *id) {
  const char *who = "hnumo_regions_create";
  if (no_engine(eng) || null_arg(eng, id, who, "id") || negative(eng, every, series_capacity, who, "every and series_capacity"))
    return HNUMO_ERR_INVALID;
  // (with_L and with_ngl dispatch these and no others; hnumo_vort_begin asks the same)
  if (eng->L < 1 || eng->L > MAXL || !sample_ngl_ok(eng->ngl))
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": unsupported nlayers or ngl (nlayers 1..3; ngl 3, 4, 5, 6 or 8), got " +
                                            std::to_string(eng->L) + ", " + std::to_string(eng->ngl));
  RegionPlan pl;
  if (int rc = region_plan(region_of_elem, n, nregions, rows_mask, eng->nelem_owned, pl, eng->err, who)) return rc;
  const int slot = free_slot(eng->regions);
  if (slot < 0)
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the engine holds " + std::to_string(RG_MAXSETS) +
                                            " region sets already (hnumo_regions_destroy frees one)");
  HIPCHK(hipSetDevice(eng->device));
  auto &s = eng->regions[slot];
  s = RegionSet{};
  const int V = rg_rows(eng->L, rows_mask), R = pl.R;
  const size_t nmem = (size_t)pl.nmem(), npoin = (size_t)eng->npoin;
  std::vector<RegionChunk> desc;
  for (const RegionPass &ps : pl.pass) desc.insert(desc.end(), ps.chunks.begin(), ps.chunks.end());
  static_assert(sizeof(RegionChunk) == sizeof(int4), "region_tree_kernel reads a descriptor as one int4");
  double *d_area = nullptr;
  bool ok = hipMalloc((void **)&s.d_mem, (nmem ? nmem : 1) * sizeof(int)) == hipSuccess &&
            hipMalloc((void **)&s.d_desc, desc.size() * sizeof(RegionChunk)) == hipSuccess &&
            alloc_doubles(&s.part, (size_t)V * nmem) && alloc_doubles(&s.lvl[0], (size_t)V * pl.level_size(0)) &&
            alloc_doubles(&s.lvl[1], (size_t)V * pl.level_size(1)) && alloc_doubles(&d_area, (size_t)R) &&
            (!(rows_mask & RG_VORT) || !coriolis_df || alloc_doubles(&s.f, npoin)) &&
            series_begin(eng, s.series, (size_t)V * R, series_capacity ? every : 0, series_capacity, false) == hipSuccess;
  ok = ok && (nmem == 0 || hipMemcpy(s.d_mem, pl.members.data(), nmem * sizeof(int), hipMemcpyHostToDevice) == hipSuccess) &&
       hipMemcpy(s.d_desc, desc.data(), desc.size() * sizeof(RegionChunk), hipMemcpyHostToDevice) == hipSuccess &&
       (!s.f || hipMemcpy(s.f, coriolis_df, npoin * sizeof(double), hipMemcpyHostToDevice) == hipSuccess);
  s.V = V;
  s.plan = std::move(pl);
  s.area.assign((size_t)R, 0.0);
  int rc = HNUMO_OK;
  if (ok) {
    // the areas: the members' sums of w_I*1.0 in node order into row 0 of part, then the same tree
    if (nmem > 0) {
      const int nb = block_count(nmem, RG_BS / eng->P);
      hipLaunchKernelGGL(region_area_kernel, dim3(nb), dim3(RG_BS), 0, eng->stream, eng->nstat + (size_t)NS_W * npoin, s.d_mem,
                         (int)nmem, eng->ngl, s.part);
    }
    regions_tree(eng, s, 1, d_area);
    ok = hipGetLastError() == hipSuccess;
    if (ok) rc = download(eng, s.area.data(), d_area, (size_t)R * sizeof(double));
  }
  (void)hipFree(d_area);
  if (!ok || rc) {
    (void)hipGetLastError();
    regions_free(eng, slot);
    return rc ? rc : fail(eng, HNUMO_ERR_DEVICE, std::string(who) + ": device allocation or upload failed");
  }
  s.plan.slot = std::vector<int32_t>();   // (the device holds the member list; the passes stay for the launches)
  s.used = true;
  regions_flag(eng);
  *id = slot;
  return HNUMO_OK;
}

// one sample of the set into its series, ordered after what is on the engine stream; no copy back
static int regions_record(hnumo_engine *eng, RegionSet &s, int id, const char *who) {
  if (no_state(eng, who) || regions_no_series(eng, s, id, who)) return HNUMO_ERR_INVALID;
  if (int rc = series_full(eng, s.series, who, "the series of region set " + std::to_string(id), "samples", "recorded")) return rc;
  const int nmem = (int)s.plan.nmem(), EPB = RG_BS / eng->P;
  if (nmem > 0) {
    RegionArgs a{};
    a.q = eng->q;
    a.alpha = eng->alpha;
    a.nstat = eng->nstat;
    a.f = s.f;
    a.dpsi = eng->basis + 2 * (size_t)eng->ngl * eng->nq;
    a.mem = s.d_mem;
    a.part = s.part;
    a.gravity = eng->p.gravity;
    a.npoin = eng->npoin;
    a.nmem = nmem;
    const int nb = block_count(nmem, EPB);
    with_ngl(eng->ngl, [&](auto ngl) {
      with_L(eng->L, [&](auto l) {
        constexpr int NGL = decltype(ngl)::value, L = decltype(l)::value;
        switch (s.plan.mask) {
          case RG_FLOW: hipLaunchKernelGGL((region_accumulate_kernel<NGL, L, RG_FLOW>), dim3(nb), dim3(RG_BS), 0, eng->stream, a); break;
          case RG_VORT: hipLaunchKernelGGL((region_accumulate_kernel<NGL, L, RG_VORT>), dim3(nb), dim3(RG_BS), 0, eng->stream, a); break;
          default:
            hipLaunchKernelGGL((region_accumulate_kernel<NGL, L, RG_FLOW | RG_VORT>), dim3(nb), dim3(RG_BS), 0, eng->stream, a);
            break;
        }
      });
    });
  }
  regions_tree(eng, s, s.V, series_slot(s.series));
  HIPCHK(hipGetLastError());
  s.series.count++;
  return HNUMO_OK;
}

extern "C" int hnumo_regions_sample(hnumo_engine *eng, int32_t id) {
  auto *s = regions_set(eng, id, "hnumo_regions_sample");
  if (!s) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  return regions_record(eng, *s, id, "hnumo_regions_sample");
}

extern "C" int hnumo_regions_series(hnumo_engine *eng, int32_t id, double *out, int64_t n, int64_t *count, int32_t clear) {
  const char *who = "hnumo_regions_series";
  auto *s = regions_set(eng, id, who);
  if (!s || regions_no_series(eng, *s, id, who)) return HNUMO_ERR_INVALID;
  return series_read(eng, s->series, s->V, (size_t)s->plan.R, out, n, count, clear, who, "V*nregions");
}

extern "C" int hnumo_regions_area(hnumo_engine *eng, int32_t id, double *out, int64_t n) {
  const char *who = "hnumo_regions_area";
  const auto *s = regions_set(eng, id, who);
  if (!s || null_arg(eng, out, who, "out") || wrong_n(eng, n, s->plan.R, who, "the set's nregions")) return HNUMO_ERR_INVALID;
  std::memcpy(out, s->area.data(), (size_t)n * sizeof(double));
  return HNUMO_OK;
}

extern "C" int hnumo_regions_destroy(hnumo_engine *eng, int32_t id) {
  if (!regions_set(eng, id, "hnumo_regions_destroy")) return HNUMO_ERR_INVALID;
  if (int rc = drain(eng)) return rc;  // (a sample in flight uses the set's tables)
  regions_free(eng, id);
  return HNUMO_OK;
}

// ------------------------------------------------------------------ sample sets
// eng->samples[]: the host plan (sample_plan.h), its tables on the device, one sample's output [V][M]
// and the series [capacity][V][M]
using SampleSet = hnumo_engine::SampleSet;

static void sample_free(hnumo_engine *eng, int id) {
  auto &s = eng->samples[id];
  dfree(s.d_tab, s.d_w, s.d_out);
  series_free(s.series);
  s = SampleSet{};
}

static SampleSet *sample_set(hnumo_engine *eng, int32_t id, const char *who) {
  return no_engine(eng) ? nullptr : set_by_id(eng, eng->samples, id, who, "sample");
}

// the located or given points of `pl` become a set: tables built and uploaded
static int sample_adopt(hnumo_engine *eng, SamplePlan &pl, const double *xgl, int32_t source, int32_t *id, const char *who) {
  const int slot = free_slot(eng->samples);
  if (slot < 0)
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the engine holds " + std::to_string(SP_MAXSETS) +
                                            " sample sets already (hnumo_sample_destroy frees one)");
  const int V = sp_nval(eng->L, source);
  sample_chunks(xgl, sp_K(eng->ngl, V), pl);
  HIPCHK(hipSetDevice(eng->device));
  auto &s = eng->samples[slot];
  s = SampleSet{};
  const size_t M = (size_t)pl.M, nch = (size_t)pl.nchunks(), nel = pl.el_list.size();
  const size_t ntab = 2 * (nch + 1) + nel + 2 * M;
  std::vector<int> tab;
  tab.reserve(ntab);
  for (const std::vector<int32_t> *v : {&pl.chunk_pt, &pl.chunk_el, &pl.el_list, &pl.slot, &pl.perm})
    tab.insert(tab.end(), v->begin(), v->end());
  bool ok = hipMalloc((void **)&s.d_tab, ntab * sizeof(int)) == hipSuccess &&
            hipMalloc((void **)&s.d_w, pl.w.size() * sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&s.d_out, (size_t)V * M * sizeof(double)) == hipSuccess;
  ok = ok && hipMemcpy(s.d_tab, tab.data(), ntab * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(s.d_w, pl.w.data(), pl.w.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    sample_free(eng, slot);
    return fail(eng, HNUMO_ERR_DEVICE, std::string(who) + ": device allocation or upload failed");
  }
  s.d_chunk_pt = s.d_tab;
  s.d_chunk_el = s.d_chunk_pt + nch + 1;
  s.d_el_list = s.d_chunk_el + nch + 1;
  s.d_slot = s.d_el_list + nel;
  s.d_perm = s.d_slot + M;
  s.source = source;
  s.V = V;
  s.plan = std::move(pl);
  s.plan.w = std::vector<double>();   // (the device holds the weights and the work lists)
  s.plan.slot = s.plan.perm = std::vector<int32_t>();
  s.used = true;
  *id = slot;
  return HNUMO_OK;
}

static int sample_create_checks(hnumo_engine *eng, int32_t source, const int32_t *id, const char *who) {
  if (no_engine(eng) || null_arg(eng, id, who, "id")) return HNUMO_ERR_INVALID;
  if (source != HNUMO_SAMPLE_STATE && source != HNUMO_SAMPLE_STATS && source != HNUMO_SAMPLE_VORT && source != HNUMO_SAMPLE_COV)
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": source must be HNUMO_SAMPLE_STATE, HNUMO_SAMPLE_STATS, " +
                                            "HNUMO_SAMPLE_VORT or HNUMO_SAMPLE_COV, got " + std::to_string(source));
  if (source == HNUMO_SAMPLE_VORT && !eng->vort.on)
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": a set on the vorticity products needs f: call hnumo_vort_begin first");
  if (source == HNUMO_SAMPLE_COV && !eng->cov.on)
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the set samples the eddy covariances: call hnumo_cov_begin first");
  if (eng->L < 1 || eng->L > MAXL || !sample_ngl_ok(eng->ngl))
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": unsupported nlayers or ngl");
  return 0;
}

extern "C" int hnumo_sample_create(hnumo_engine *eng, const double *coord, int32_t ldc, const double *xgl, const double *xy,
                                   int64_t M, int32_t source, int32_t *id) {
  if (int rc = sample_create_checks(eng, source, id, "hnumo_sample_create")) return rc;
  SamplePlan pl;
  if (int rc = sample_locate(coord, ldc, xgl, eng->ngl, eng->nelem_owned, xy, M, pl, eng->err)) return rc;
  return sample_adopt(eng, pl, xgl, source, id, "hnumo_sample_create");
}

extern "C" int hnumo_sample_create_ref(hnumo_engine *eng, const double *xgl, const int32_t *elem, const double *xi_eta,
                                       int64_t M, int32_t source, int32_t *id) {
  if (int rc = sample_create_checks(eng, source, id, "hnumo_sample_create_ref")) return rc;
  SamplePlan pl;
  if (int rc = sample_take_ref(xgl, eng->ngl, eng->nelem_owned, elem, xi_eta, M, pl, eng->err)) return rc;
  return sample_adopt(eng, pl, xgl, source, id, "hnumo_sample_create_ref");
}

extern "C" int hnumo_sample_plan(hnumo_engine *eng, int32_t id, int32_t *elem, double *xi_eta, int64_t M) {
  const auto *s = sample_set(eng, id, "hnumo_sample_plan");
  if (!s || wrong_M(eng, M, s->plan.M, "hnumo_sample_plan")) return HNUMO_ERR_INVALID;
  if (elem) std::memcpy(elem, s->plan.elem.data(), (size_t)M * sizeof(int32_t));
  if (xi_eta) std::memcpy(xi_eta, s->plan.xi_eta.data(), 2 * (size_t)M * sizeof(double));
  return HNUMO_OK;
}

// one sample of the set into `dst` [V][M] on the device, ordered after what is on the engine stream
static int sample_now(hnumo_engine *eng, const SampleSet &s, double *dst, const char *who) {
  if (no_state(eng, who)) return HNUMO_ERR_INVALID;
  if (s.source == HNUMO_SAMPLE_STATS) {
    if (!eng->stats.on) return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the set samples the flow statistics: call hnumo_stats_begin first");
    if (eng->stats.nsamples == 0) return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the flow statistics have no samples yet");
  }
  if (s.source == HNUMO_SAMPLE_VORT && !eng->vort.on)
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the set samples the vorticity products, which need f: call hnumo_vort_begin first");
  if (s.source == HNUMO_SAMPLE_COV) {
    if (!eng->cov.on) return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the set samples the eddy covariances: call hnumo_cov_begin first");
    if (eng->cov.nsamples == 0) return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the eddy covariances have no samples yet");
  }
  SampleArgs a{};
  a.nstat = eng->nstat;
  a.f = eng->vort.f;
  a.dpsi = eng->basis + 2 * (size_t)eng->ngl * eng->nq;
  a.q = eng->q;
  a.qb = eng->qb;
  a.zbot = eng->nstat + (size_t)NS_ZB * eng->npoin;
  a.alpha = eng->alpha;
  a.sums = (const double2 *)eng->stats.sums;
  a.gravity = eng->p.gravity;
  a.nsamp = (double)eng->stats.nsamples;
  a.chunk_pt = s.d_chunk_pt;
  a.chunk_el = s.d_chunk_el;
  a.el_list = s.d_el_list;
  a.slot = s.d_slot;
  a.perm = s.d_perm;
  a.w = s.d_w;
  a.out = dst;
  a.npoin = (size_t)eng->npoin;
  a.M = (size_t)s.plan.M;
  const int nch = s.plan.nchunks();
  if (s.source == HNUMO_SAMPLE_COV) {
    // (the fields of the covariances' own sums and sample count, as STATS reads the statistics')
    a.sums = (const double2 *)eng->cov.sums;
    a.nsamp = (double)eng->cov.nsamples;
    with_ngl(eng->ngl, [&](auto ngl) {
      cov_with_L(eng->L, [&](auto l) {
        constexpr int NGL = decltype(ngl)::value, L = decltype(l)::value;
        hipLaunchKernelGGL((sample_kernel<NGL, L, SP_SRC_COV>), dim3(nch), dim3(SP_CHUNK), 0, eng->stream, a);
      });
    });
    HIPCHK(hipGetLastError());
    return HNUMO_OK;
  }
  with_ngl(eng->ngl, [&](auto ngl) {
    with_L(eng->L, [&](auto l) {
      constexpr int NGL = decltype(ngl)::value, L = decltype(l)::value;
      if (s.source == HNUMO_SAMPLE_VORT)
        hipLaunchKernelGGL((sample_kernel<NGL, L, SP_SRC_VORT>), dim3(nch), dim3(SP_CHUNK), 0, eng->stream, a);
      else if (s.source == HNUMO_SAMPLE_STATS)
        hipLaunchKernelGGL((sample_kernel<NGL, L, SP_SRC_STATS>), dim3(nch), dim3(SP_CHUNK), 0, eng->stream, a);
      else
        hipLaunchKernelGGL((sample_kernel<NGL, L, SP_SRC_STATE>), dim3(nch), dim3(SP_CHUNK), 0, eng->stream, a);
    });
  });
  HIPCHK(hipGetLastError());
  return HNUMO_OK;
}

extern "C" int hnumo_sample(hnumo_engine *eng, int32_t id, double *out, int64_t n) {
  const char *who = "hnumo_sample";
  auto *s = sample_set(eng, id, who);
  if (!s || null_arg(eng, out, who, "out")) return HNUMO_ERR_INVALID;
  const int64_t want = (int64_t)s->V * s->plan.M;
  if (wrong_n(eng, n, want, who, "V*M")) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  if (int rc = sample_now(eng, *s, s->d_out, who)) return rc;
  std::vector<double> raw((size_t)want);
  if (int rc = download(eng, raw.data(), s->d_out, (size_t)want * sizeof(double))) return rc;
  sample_transpose(raw.data(), s->V, (size_t)s->plan.M, 1, out);
  return HNUMO_OK;
}

extern "C" int hnumo_sample_series_begin(hnumo_engine *eng, int32_t id, int32_t every, int32_t capacity) {
  const char *who = "hnumo_sample_series_begin";
  auto *s = sample_set(eng, id, who);
  if (!s || negative(eng, every, capacity, who, "every and capacity")) return HNUMO_ERR_INVALID;
  if (int rc = drain(eng)) return rc;  // (a recording in flight writes the old series)
  // (no series: nothing to record into, so nothing is due after a step either)
  if (series_begin(eng, s->series, (size_t)s->V * (size_t)s->plan.M, capacity ? every : 0, capacity, false) != hipSuccess)
    return fail(eng, HNUMO_ERR_DEVICE, "hnumo_sample_series_begin: device allocation failed");
  return HNUMO_OK;
}

static int sample_record(hnumo_engine *eng, SampleSet &s, int id, const char *who) {
  if (int rc = series_full(eng, s.series, who, "the series of sample set " + std::to_string(id), "samples", "recorded")) return rc;
  if (int rc = sample_now(eng, s, series_slot(s.series), who)) return rc;
  s.series.count++;
  return HNUMO_OK;
}

extern "C" int hnumo_sample_record(hnumo_engine *eng, int32_t id) {
  auto *s = sample_set(eng, id, "hnumo_sample_record");
  if (!s) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  return sample_record(eng, *s, id, "hnumo_sample_record");
}

extern "C" int hnumo_sample_series(hnumo_engine *eng, int32_t id, double *out, int64_t n, int64_t *count, int32_t clear) {
  auto *s = sample_set(eng, id, "hnumo_sample_series");
  if (!s) return HNUMO_ERR_INVALID;
  return series_read(eng, s->series, s->V, (size_t)s->plan.M, out, n, count, clear, "hnumo_sample_series", "V*M");
}

extern "C" int hnumo_sample_destroy(hnumo_engine *eng, int32_t id) {
  if (!sample_set(eng, id, "hnumo_sample_destroy")) return HNUMO_ERR_INVALID;
  if (int rc = drain(eng)) return rc;  // (a sample in flight uses the set's tables)
  sample_free(eng, id);
  return HNUMO_OK;
}

// ------------------------------------------------------------------ float sets
// eng->floats[]: the host geometry (float_plan.h; hnumo_floats_set locates in it), the permutation
// back to input order, the element tables and the SoA floats on the device, the series
// [capacity][5 + S][M] (S: the rows of the set's sensor mask).  The floats' own rules sit on top of the Series: `every` (0 or 1) is whether the
// engine advances the set after a step; the series counts advances, not steps, and its every is the
// caller's record_every
using FloatSet = hnumo_engine::FloatSet;

static void floats_free(hnumo_engine *eng, int id) {
  auto &s = eng->floats[id];
  dfree(s.d_geo, s.d_nbr, s.d_f, s.d_i, s.d_mig, s.d_boxi);
  dfree(s.d_boxd, s.d_sense);
  series_free(s.series);
  s = FloatSet{};
}

static FloatSet *floats_set(hnumo_engine *eng, int32_t id, const char *who) {
  return no_engine(eng) ? nullptr : set_by_id(eng, eng->floats, id, who, "float");
}

// the plan's floats (sorted order) to the device
static bool floats_upload(FloatSet &s, const FloatPlan &pl) {
  const size_t M = (size_t)pl.M;
  bool ok = true;
  const std::vector<double> *fd[6] = {&pl.x, &pl.y, &pl.wx, &pl.wy, &pl.xi, &pl.eta};
  for (int v = 0; v < 6; v++) ok = ok && hipMemcpy(s.d_f + v * M, fd[v]->data(), M * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  const std::vector<int32_t> *id[5] = {&pl.elem, &pl.layer, &pl.status, &pl.fresh, &pl.perm};
  for (int v = 0; v < 5; v++) ok = ok && hipMemcpy(s.d_i + v * M, id[v]->data(), M * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
  return ok;
}

extern "C" int hnumo_floats_create(hnumo_engine *eng, const double *coord, int32_t ldc, const double *xgl, const double *xy,
                                   const int32_t *layer, int64_t M, int32_t *id) {
  const char *who = "hnumo_floats_create";
  if (no_engine(eng) || null_arg(eng, id, who, "id")) return HNUMO_ERR_INVALID;
  if (eng->L < 1 || eng->L > MAXL || !float_ngl_ok(eng->ngl))
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": unsupported nlayers or ngl");
  if (!eng->fl_nbr_err.empty()) return fail(eng, HNUMO_ERR_INVALID, eng->fl_nbr_err);
  const int slot = free_slot(eng->floats);
  if (slot < 0)
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the engine holds " + std::to_string(FL_MAXSETS) +
                                            " float sets already (hnumo_floats_destroy frees one)");
  FloatGeom geom;
  if (int rc = float_geometry(coord, ldc, xgl, eng->ngl, eng->nelem_owned, eng->fl_nbr, geom, eng->err)) return rc;
  FloatPlan pl;
  if (int rc = float_seed(geom, eng->L, xy, layer, M, pl, eng->err, who)) return rc;
  HIPCHK(hipSetDevice(eng->device));
  auto &s = eng->floats[slot];
  s = FloatSet{};
  const size_t ne = (size_t)geom.ne, m = (size_t)M;
  bool ok = hipMalloc((void **)&s.d_geo, (9 * ne + 1) * sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&s.d_nbr, (4 * ne + 1) * sizeof(int)) == hipSuccess &&
            hipMalloc((void **)&s.d_f, 6 * m * sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&s.d_i, 5 * m * sizeof(int)) == hipSuccess;
  if (ok && ne > 0)
    ok = hipMemcpy(s.d_geo, geom.corners.data(), 8 * ne * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(s.d_geo + 8 * ne, geom.tol.data(), ne * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(s.d_nbr, geom.nbr.data(), 4 * ne * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && floats_upload(s, pl);
  if (!ok) {
    (void)hipGetLastError();
    floats_free(eng, slot);
    return fail(eng, HNUMO_ERR_DEVICE, std::string(who) + ": device allocation or upload failed");
  }
  s.M = M;
  s.geom = std::move(geom);
  s.perm = std::move(pl.perm);
  s.used = true;
  *id = slot;
  return HNUMO_OK;
}

// the inverse permutation of a migrating set, behind xface and arrive in d_mig
static bool floats_upload_iperm(hnumo_engine *eng, FloatSet &s) {
  const std::vector<int32_t> ip = float_inverse_perm(s.perm);
  return hipMemcpy(s.d_mig + eng->fl_xface.size() + eng->fl_arrive.size(), ip.data(), ip.size() * sizeof(int), hipMemcpyHostToDevice) ==
         hipSuccess;
}

extern "C" int hnumo_floats_set(hnumo_engine *eng, int32_t id, const double *xy, const int32_t *layer, int64_t M) {
  auto *s = floats_set(eng, id, "hnumo_floats_set");
  if (!s || wrong_M(eng, M, s->M, "hnumo_floats_set")) return HNUMO_ERR_INVALID;
  FloatPlan pl;
  if (int rc = float_seed(s->geom, eng->L, xy, layer, M, pl, eng->err, "hnumo_floats_set")) return rc;
  if (int rc = drain(eng)) return rc;  // (an advance in flight writes the old floats)
  if (!floats_upload(*s, pl)) {
    (void)hipGetLastError();
    return fail(eng, HNUMO_ERR_DEVICE, "hnumo_floats_set: upload failed");
  }
  s->perm = std::move(pl.perm);
  if (s->mig && !floats_upload_iperm(eng, *s)) return fail(eng, HNUMO_ERR_DEVICE, "hnumo_floats_set: upload failed");
  return HNUMO_OK;
}

static FloatArgs floats_args(hnumo_engine *eng, const FloatSet &s) {
  FloatArgs a{};
  const size_t ne = (size_t)s.geom.ne, M = (size_t)s.M;
  a.f.corners = s.d_geo;
  a.f.tol = s.d_geo + 8 * ne;
  a.f.nbr = s.d_nbr;
  a.f.q = eng->q;
  a.f.npoin = (size_t)eng->npoin;
  for (int i = 0; i < s.geom.ngl; i++) a.f.xgl[i] = s.geom.xgl[i];
  a.x = s.d_f, a.y = s.d_f + M, a.wx = s.d_f + 2 * M, a.wy = s.d_f + 3 * M, a.xi = s.d_f + 4 * M, a.eta = s.d_f + 5 * M;
  a.elem = s.d_i, a.layer = s.d_i + M, a.status = s.d_i + 2 * M, a.fresh = s.d_i + 3 * M, a.perm = s.d_i + 4 * M;
  a.M = M;
  return a;
}

// ---- sensors: S rows behind the 5 of a record (float_sense_kernel)
static int floats_nrows(const FloatSet &s) { return FL_NREC + fl_sense_rows(s.sensors); }

// why the set's sensors cannot be read now, or 0
static int floats_sense_refused(hnumo_engine *eng, const FloatSet &s, const char *who) {
  if (!eng->has_state)
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the set's sensors read the state and there is none on the device yet (run a step first)");
  if ((s.sensors & FL_SENSE_VORT) && !eng->vort.on)
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the set's sensors hold HNUMO_FLOAT_SENSE_VORT, which needs f: hnumo_vort_end "
                                            "has been called (call hnumo_vort_begin again)");
  return 0;
}

// the S sensor rows of the set into dst [S][M] on the device (input order), ordered after what is on the engine stream
static int floats_sense_launch(hnumo_engine *eng, const FloatSet &s, double *dst) {
  const FloatArgs f = floats_args(eng, s);
  FloatSenseArgs a{};
  a.g.q = eng->q;
  a.g.zbot = eng->nstat + (size_t)NS_ZB * eng->npoin;
  a.g.alpha = eng->alpha;
  a.g.ex = eng->nstat + (size_t)NS_EX * eng->npoin;
  a.g.ey = eng->nstat + (size_t)NS_EY * eng->npoin;
  a.g.nx = eng->nstat + (size_t)NS_NX * eng->npoin;
  a.g.ny = eng->nstat + (size_t)NS_NY * eng->npoin;
  a.g.f = eng->vort.f;
  a.g.dpsi = eng->basis + 2 * (size_t)eng->ngl * eng->nq;
  a.g.gravity = eng->p.gravity;
  a.g.npoin = (size_t)eng->npoin;
  for (int i = 0; i < s.geom.ngl; i++) a.g.xgl[i] = s.geom.xgl[i];
  a.xi = f.xi, a.eta = f.eta, a.elem = f.elem, a.layer = f.layer, a.perm = f.perm;
  a.out = dst;
  a.M = f.M;
  const dim3 grid((unsigned)((a.M + FL_BLOCK - 1) / FL_BLOCK));
  with_ngl(eng->ngl, [&](auto ngl) {
    float_with_L_mask(eng->L, s.sensors, [&](auto l, auto m) {
      constexpr int NGL = decltype(ngl)::value, L = decltype(l)::value, MASK = decltype(m)::value;
      hipLaunchKernelGGL((float_sense_kernel<NGL, L, MASK>), grid, dim3(FL_BLOCK), 0, eng->stream, a);
    });
  });
  HIPCHK(hipGetLastError());
  return HNUMO_OK;
}

// one record of the set into the series, ordered after what is on the engine stream
static int floats_record(hnumo_engine *eng, FloatSet &s, int id, const char *who) {
  if (int rc = series_full(eng, s.series, who, "the series of float set " + std::to_string(id), "records", "recorded")) return rc;
  if (s.sensors)
    if (int rc = floats_sense_refused(eng, s, who)) return rc;
  FloatArgs a = floats_args(eng, s);
  a.rec = series_slot(s.series);
  hipLaunchKernelGGL(float_record_kernel, dim3((unsigned)((a.M + FL_BLOCK - 1) / FL_BLOCK)), dim3(FL_BLOCK), 0, eng->stream, a);
  HIPCHK(hipGetLastError());
  if (s.sensors)
    if (int rc = floats_sense_launch(eng, s, a.rec + FL_NREC * a.M)) return rc;
  s.series.count++;
  return HNUMO_OK;
}

// box 0, 1: the outboxes (their counters behind the int planes); 2: the inbox of hnumo_floats_deliver
static FloatBox floats_box(const FloatSet &s, int which) {
  const size_t M = (size_t)s.M;
  return FloatBox{s.d_boxd + (size_t)which * FL_FD * M, s.d_boxi + (size_t)which * FL_FI * M,
                  which < 2 ? s.d_boxi + 3 * FL_FI * M + which : nullptr, M};
}

// one advance of the set on the state on the device now, and the record that is due after it
static int floats_advance(hnumo_engine *eng, FloatSet &s, int id, double dt, const char *who) {
  if (no_state(eng, who) || (!float_finite(dt) && refused(eng, who, "dt is not finite"))) return HNUMO_ERR_INVALID;
  FloatArgs a = floats_args(eng, s);
  a.dt = dt;
  if (s.mig) {
    // flights go to the outbox of the current parity; the record that falls due waits for the arrivals
    // (floats_group_advance, or hnumo_floats_settle on a host that carries the records itself)
    FloatMigArgs m{a, s.d_mig, floats_box(s, s.parity)};
    HIPCHK(hipMemsetAsync(m.out.count, 0, sizeof(int), eng->stream));
    with_ngl(eng->ngl, [&](auto ngl) {
      constexpr int NGL = decltype(ngl)::value;
      hipLaunchKernelGGL((float_advance_kernel<NGL, 1, true>), dim3((unsigned)((a.M + FL_BLOCK - 1) / FL_BLOCK)), dim3(FL_BLOCK), 0,
                         eng->stream, m);
    });
    HIPCHK(hipGetLastError());
    if (series_due(s.series)) s.settle_due = true;
    return HNUMO_OK;
  }
  with_ngl(eng->ngl, [&](auto ngl) {
    constexpr int NGL = decltype(ngl)::value, G = fl_group(NGL);
    if (eng->fl_rows)
      hipLaunchKernelGGL((float_advance_kernel<NGL, G, false>), dim3((unsigned)((a.M * G + FL_BLOCK - 1) / FL_BLOCK)), dim3(FL_BLOCK), 0,
                         eng->stream, a);
    else
      hipLaunchKernelGGL((float_advance_kernel<NGL, 1, false>), dim3((unsigned)((a.M + FL_BLOCK - 1) / FL_BLOCK)), dim3(FL_BLOCK), 0,
                         eng->stream, a);
  });
  HIPCHK(hipGetLastError());
  if (series_due(s.series)) return floats_record(eng, s, id, who);
  return HNUMO_OK;
}

extern "C" int hnumo_floats_advance(hnumo_engine *eng, int32_t id, double dt) {
  auto *s = floats_set(eng, id, "hnumo_floats_advance");
  if (!s) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  return floats_advance(eng, *s, id, dt, "hnumo_floats_advance");
}

extern "C" int hnumo_floats_begin(hnumo_engine *eng, int32_t id, int32_t every, int32_t record_every, int32_t capacity) {
  const char *who = "hnumo_floats_begin";
  auto *s = floats_set(eng, id, who);
  if (!s) return HNUMO_ERR_INVALID;
  if (every != 0 && every != 1)
    return fail(eng, HNUMO_ERR_INVALID, "hnumo_floats_begin: every must be 0 or 1 (a float cannot skip steps), got " + std::to_string(every));
  if (negative(eng, record_every, capacity, who, "record_every and capacity")) return HNUMO_ERR_INVALID;
  if (int rc = drain(eng)) return rc;  // (a record in flight writes the old series)
  s->every = 0;
  s->settle_due = false;
  // (record_every holds with capacity 0 too: the record that falls due is then refused as into a full series)
  if (series_begin(eng, s->series, (size_t)floats_nrows(*s) * (size_t)s->M, record_every, capacity, false) != hipSuccess)
    return fail(eng, HNUMO_ERR_DEVICE, "hnumo_floats_begin: device allocation failed");
  s->every = every;
  return HNUMO_OK;
}

extern "C" int hnumo_floats_record(hnumo_engine *eng, int32_t id) {
  auto *s = floats_set(eng, id, "hnumo_floats_record");
  if (!s) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  return floats_record(eng, *s, id, "hnumo_floats_record");
}

extern "C" int hnumo_floats_get(hnumo_engine *eng, int32_t id, double *x, double *y, double *u, double *v, int32_t *elem,
                                int32_t *status, int64_t M) {
  auto *s = floats_set(eng, id, "hnumo_floats_get");
  if (!s || wrong_M(eng, M, s->M, "hnumo_floats_get")) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  const size_t m = (size_t)M;
  std::vector<double> fd(4 * m);
  std::vector<int32_t> fi(3 * m);
  if (int rc = download(eng, fd.data(), s->d_f, 4 * m * sizeof(double))) return rc;
  if (int rc = download(eng, fi.data(), s->d_i, 3 * m * sizeof(int))) return rc;
  double *od[4] = {x, y, u, v};
  for (size_t t = 0; t < m; t++) {
    const size_t p = (size_t)s->perm[t];
    for (int c = 0; c < 4; c++)
      if (od[c]) od[c][p] = fd[c * m + t];
    if (elem) elem[p] = fi[t];
    if (status) status[p] = fi[2 * m + t];
  }
  return HNUMO_OK;
}

extern "C" int hnumo_floats_plan(hnumo_engine *eng, int32_t id, int32_t *elem, double *xi_eta, int64_t M) {
  auto *s = floats_set(eng, id, "hnumo_floats_plan");
  if (!s || wrong_M(eng, M, s->M, "hnumo_floats_plan")) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  const size_t m = (size_t)M;
  std::vector<double> fd(2 * m);
  std::vector<int32_t> fi(m);
  if (int rc = download(eng, fd.data(), s->d_f + 4 * m, 2 * m * sizeof(double))) return rc;
  if (int rc = download(eng, fi.data(), s->d_i, m * sizeof(int))) return rc;
  for (size_t t = 0; t < m; t++) {
    const size_t p = (size_t)s->perm[t];
    if (elem) elem[p] = fi[t];
    if (xi_eta) xi_eta[2 * p] = fd[t], xi_eta[2 * p + 1] = fd[m + t];
  }
  return HNUMO_OK;
}

extern "C" int hnumo_floats_series(hnumo_engine *eng, int32_t id, double *out, int64_t n, int64_t *count, int32_t clear) {
  auto *s = floats_set(eng, id, "hnumo_floats_series");
  if (!s) return HNUMO_ERR_INVALID;
  return series_read(eng, s->series, floats_nrows(*s), (size_t)s->M, out, n, count, clear, "hnumo_floats_series",
                     s->sensors ? "(5+S)*M" : "5*M");
}

extern "C" int hnumo_floats_sensors(hnumo_engine *eng, int32_t id, int32_t mask) {
  const char *who = "hnumo_floats_sensors";
  auto *s = floats_set(eng, id, who);
  if (!s) return HNUMO_ERR_INVALID;
  if (mask < 0 || (mask & ~FL_SENSE_ALL))
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": mask must be a sum of HNUMO_FLOAT_SENSE_STATE (1) and HNUMO_FLOAT_SENSE_VORT (2), got " +
                                            std::to_string(mask));
  if ((mask & FL_SENSE_VORT) && !eng->vort.on)
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": HNUMO_FLOAT_SENSE_VORT needs f: call hnumo_vort_begin first");
  if (s->series.cap > 0 && fl_sense_rows(mask) != fl_sense_rows(s->sensors))
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the series of float set " + std::to_string(id) + " holds records of " +
                                            std::to_string(floats_nrows(*s)) + " rows, the mask asks for " +
                                            std::to_string(FL_NREC + fl_sense_rows(mask)) +
                                            ": call hnumo_floats_begin with capacity 0 first, then hnumo_floats_sensors, then hnumo_floats_begin");
  if (int rc = drain(eng)) return rc;  // (a record in flight runs the old mask's kernel)
  s->sensors = mask;
  if (s->series.cap == 0) s->series.width = (size_t)floats_nrows(*s) * (size_t)s->M;
  return HNUMO_OK;
}

extern "C" int hnumo_floats_sense_info(hnumo_engine *eng, int32_t id, int32_t *nrows, int32_t *K) {
  auto *s = floats_set(eng, id, "hnumo_floats_sense_info");
  if (!s) return HNUMO_ERR_INVALID;
  if (nrows) *nrows = fl_sense_rows(s->sensors);
  if (K) {
    *K = 0;
    if (s->sensors)
      with_ngl(eng->ngl, [&](auto ngl) {
        float_with_L_mask(eng->L, s->sensors, [&](auto l, auto m) {
          *K = fl_sense_K(decltype(ngl)::value, decltype(l)::value, decltype(m)::value);
        });
      });
  }
  return HNUMO_OK;
}

extern "C" int hnumo_floats_sense(hnumo_engine *eng, int32_t id, double *out, int64_t n) {
  const char *who = "hnumo_floats_sense";
  auto *s = floats_set(eng, id, who);
  if (!s) return HNUMO_ERR_INVALID;
  const int S = fl_sense_rows(s->sensors);
  if (S == 0) return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": float set " + std::to_string(id) + " has no sensors (hnumo_floats_sensors)");
  const int64_t want = (int64_t)S * s->M;
  if (null_arg(eng, out, who, "out") || wrong_n(eng, n, want, who, "S*M")) return HNUMO_ERR_INVALID;
  if (int rc = floats_sense_refused(eng, *s, who)) return rc;
  HIPCHK(hipSetDevice(eng->device));
  // (sized for every sensor: the mask may change)
  if (!s->d_sense && !alloc_doubles(&s->d_sense, (size_t)fl_sense_rows(FL_SENSE_ALL) * (size_t)s->M)) {
    (void)hipGetLastError();
    return fail(eng, HNUMO_ERR_DEVICE, std::string(who) + ": device allocation failed");
  }
  if (int rc = floats_sense_launch(eng, *s, s->d_sense)) return rc;
  std::vector<double> raw((size_t)want);
  if (int rc = download(eng, raw.data(), s->d_sense, (size_t)want * sizeof(double))) return rc;
  sample_transpose(raw.data(), S, (size_t)s->M, 1, out);
  return HNUMO_OK;
}

extern "C" int hnumo_floats_destroy(hnumo_engine *eng, int32_t id) {
  if (!floats_set(eng, id, "hnumo_floats_destroy")) return HNUMO_ERR_INVALID;
  if (int rc = drain(eng)) return rc;  // (an advance in flight uses the set's tables)
  floats_free(eng, id);
  return HNUMO_OK;
}

// ------------------------------------------------------------------ float sets: migration between ranks
// the index of `rank` among eng's processor-face neighbours, or -1
static int floats_nb_index(const hnumo_engine *eng, int rank) {
  for (size_t k = 0; k < eng->fnb.size(); k++)
    if (eng->fnb[k].rank == rank) return (int)k;
  return -1;
}

// the tol_e the set locates with from now on: the rank's own, or those of coord_scale
static int floats_upload_tol(hnumo_engine *eng, FloatSet &s, double scale) {
  std::vector<double> tol = s.geom.tol;
  if (scale > 0.0) float_tolerances(s.geom.corners, scale, tol);
  HIPCHK(hipStreamSynchronize(eng->stream));  // (an advance in flight reads the old ones)
  if (!tol.empty()) HIPCHK(hipMemcpy(s.d_geo + 8 * tol.size(), tol.data(), tol.size() * sizeof(double), hipMemcpyHostToDevice));
  s.coord_scale = scale;
  return HNUMO_OK;
}

static int floats_migrate(hnumo_engine *eng, int32_t id, int32_t on, double scale, const char *who) {
  auto *s = floats_set(eng, id, who);
  if (!s) return HNUMO_ERR_INVALID;
  if (!eng->face_halo || eng->nranks < 2)
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": floats migrate across processor faces: the engine needs a processor-face "
                                            "halo with nranks > 1 (not a single rank, a ghost-layer partition or the self-neighbour emulation)");
  if (!(scale >= 0.0) || !float_finite(scale))
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": coord_scale must be finite and >= 0");
  if (!eng->fl_xface_err.empty()) return fail(eng, HNUMO_ERR_INVALID, eng->fl_xface_err);
  HIPCHK(hipSetDevice(eng->device));
  if (on && !s->d_mig) {
    const size_t M = (size_t)s->M, nx = eng->fl_xface.size(), na = eng->fl_arrive.size();
    bool ok = hipMalloc((void **)&s->d_mig, (nx + na + M) * sizeof(int)) == hipSuccess &&
              hipMalloc((void **)&s->d_boxd, 3 * FL_FD * M * sizeof(double)) == hipSuccess &&
              hipMalloc((void **)&s->d_boxi, (3 * FL_FI * M + 2) * sizeof(int)) == hipSuccess;
    ok = ok && (nx == 0 || hipMemcpy(s->d_mig, eng->fl_xface.data(), nx * sizeof(int), hipMemcpyHostToDevice) == hipSuccess) &&
         (na == 0 || hipMemcpy(s->d_mig + nx, eng->fl_arrive.data(), na * sizeof(int), hipMemcpyHostToDevice) == hipSuccess) &&
         floats_upload_iperm(eng, *s) && hipMemset(s->d_boxi + 3 * FL_FI * M, 0, 2 * sizeof(int)) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      dfree(s->d_mig, s->d_boxi);
      dfree(s->d_boxd);
      return fail(eng, HNUMO_ERR_DEVICE, std::string(who) + ": device allocation or upload failed");
    }
  }
  if (int rc = floats_upload_tol(eng, *s, on ? scale : 0.0)) return rc;
  s->mig = on != 0;
  s->settle_due = false;
  return HNUMO_OK;
}

extern "C" int hnumo_floats_migrate(hnumo_engine *eng, int32_t id, int32_t on, double coord_scale) {
  return floats_migrate(eng, id, on, coord_scale, "hnumo_floats_migrate");
}

// floats idx[0..n) (input positions) become `status` where they are, elem 0, w 0 (float_mark_kernel); d_idx: on the device
static int floats_mark(hnumo_engine *eng, FloatSet &s, const int *d_idx, int n, int status) {
  if (n <= 0) return HNUMO_OK;
  FloatMarkArgs g{floats_args(eng, s), d_idx, s.d_mig + eng->fl_xface.size() + eng->fl_arrive.size(), n, status};
  hipLaunchKernelGGL(float_mark_kernel, dim3((unsigned)((n + FL_BLOCK - 1) / FL_BLOCK)), dim3(FL_BLOCK), 0, eng->stream, g);
  HIPCHK(hipGetLastError());
  return HNUMO_OK;
}

static int floats_release(hnumo_engine *eng, FloatSet &s, const int32_t *idx, int64_t n, const char *who) {
  if (n < 0 || (n > 0 && !idx)) return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": idx is NULL or n < 0");
  if (!s.mig) return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the set does not migrate (hnumo_floats_migrate)");
  for (int64_t t = 0; t < n; t++)
    if (idx[t] < 0 || idx[t] >= s.M)
      return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": idx(" + std::to_string(t + 1) + ") is outside 0..M-1");
  if (n == 0) return HNUMO_OK;
  // (the inbox's gid plane carries the list; nothing else uses the inbox between two calls)
  FloatBox in = floats_box(s, 2);
  HIPCHK(hipStreamSynchronize(eng->stream));
  HIPCHK(hipMemcpy(in.i, idx, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  if (int rc = floats_mark(eng, s, in.i, (int)n, FL_LEFT)) return rc;
  HIPCHK(hipStreamSynchronize(eng->stream));
  return HNUMO_OK;
}

extern "C" int hnumo_floats_release(hnumo_engine *eng, int32_t id, const int32_t *idx, int64_t n) {
  auto *s = floats_set(eng, id, "hnumo_floats_release");
  if (!s) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  return floats_release(eng, *s, idx, n, "hnumo_floats_release");
}

// the arrivals on eng of the n entries of `in` whose k is want_k; they come across the faces eng shares with its
// neighbour `from`; flights that go on are appended to eng's outbox of the other parity
static int floats_arrive(hnumo_engine *eng, FloatSet &s, const FloatBox &in, int n, int want_k, int from) {
  if (n <= 0) return HNUMO_OK;
  FloatArriveArgs g{};
  g.a = floats_args(eng, s);
  g.xface = s.d_mig;
  g.arrive = s.d_mig + eng->fl_xface.size() + eng->fnb[from].off;
  g.iperm = s.d_mig + eng->fl_xface.size() + eng->fl_arrive.size();
  g.in = in;
  g.out = floats_box(s, s.parity ^ 1);
  g.n = n;
  g.want_k = want_k;
  g.nfaces = eng->fnb[from].n;
  g.nlayers = eng->L;
  with_ngl(eng->ngl, [&](auto ngl) {
    hipLaunchKernelGGL((float_arrive_kernel<decltype(ngl)::value>), dim3((unsigned)((n + FL_BLOCK - 1) / FL_BLOCK)), dim3(FL_BLOCK), 0,
                       eng->stream, g);
  });
  HIPCHK(hipGetLastError());
  return HNUMO_OK;
}

// the record an advance of a migrating set deferred
static int floats_settle(hnumo_engine *eng, FloatSet &s, int id, const char *who) {
  if (!s.settle_due) return HNUMO_OK;
  s.settle_due = false;
  return floats_record(eng, s, id, who);
}

// every engine holds the set `id` with the same M (and it migrates), or the refusal, on the engine at fault
static int floats_group_sets(hnumo_engine **engines, int n, int32_t id, const char *who, bool need_mig) {
  for (int i = 0; i < n; i++) {
    auto *s = floats_set(engines[i], id, who);
    if (!s) return HNUMO_ERR_INVALID;
    if (s->M != engines[0]->floats[id].M)
      return fail(engines[i], HNUMO_ERR_INVALID, std::string(who) + ": float set " + std::to_string(id) + " has another M on rank " +
                                                     std::to_string(i) + " than on rank 0 (every rank creates it from the same xy)");
    if (need_mig && !s->mig)
      return fail(engines[i], HNUMO_ERR_INVALID, std::string(who) + ": float set " + std::to_string(id) + " does not migrate on rank " +
                                                     std::to_string(i) + " (hnumo_group_floats_migrate)");
  }
  return HNUMO_OK;
}

// hnumo_group_floats_migrate: the same on every engine; on: a seed ACTIVE on several ranks stays on the lowest
static int floats_group_migrate(hnumo_engine **engines, int n, int32_t id, int32_t on, double scale) {
  const char *who = "hnumo_group_floats_migrate";
  if (int rc = floats_group_sets(engines, n, id, who, false)) return rc;
  for (int i = 0; i < n; i++)
    if (int rc = floats_migrate(engines[i], id, on, scale, who)) return rc;
  if (!on) return HNUMO_OK;
  const size_t M = (size_t)engines[0]->floats[id].M;
  std::vector<char> held(M, 0);
  std::vector<int32_t> st(M), idx;
  for (int i = 0; i < n; i++) {
    if (int rc = hnumo_floats_get(engines[i], id, nullptr, nullptr, nullptr, nullptr, nullptr, st.data(), (int64_t)M)) return rc;
    idx.clear();
    for (size_t m = 0; m < M; m++)
      if (st[m] == FL_ACTIVE) {
        if (held[m]) idx.push_back((int32_t)m);
        held[m] = 1;
      }
    if (int rc = floats_release(engines[i], engines[i]->floats[id], idx.data(), (int64_t)idx.size(), who)) return rc;
  }
  return HNUMO_OK;
}

// hnumo_group_floats_advance, and the migrating sets' part of a group step: every engine's advance, then rounds of
// arrivals until no float is in flight, then the records that fell due.  The synchronisation that starts a round is
// the ordering between the engines' streams: an outbox is read only after its writer has drained, and written again
// only two rounds later.
static int floats_group_advance(hnumo_engine **engines, int n, int32_t id, double dt, const char *who) {
  if (int rc = floats_group_sets(engines, n, id, who, true)) return rc;
  for (int i = 0; i < n; i++) {
    hnumo_engine *eng = engines[i];
    HIPCHK(hipSetDevice(eng->device));
    if (int rc = floats_advance(eng, eng->floats[id], id, dt, who)) return rc;
  }
  std::vector<int> cnt(n);
  for (int round = 0;; round++) {
    bool any = false;
    for (int i = 0; i < n; i++) {
      hnumo_engine *eng = engines[i];
      if (int rc = drain(eng)) return rc;
      auto &s = eng->floats[id];
      HIPCHK(hipMemcpy(&cnt[i], floats_box(s, s.parity).count, sizeof(int), hipMemcpyDeviceToHost));
      cnt[i] = std::min<int64_t>(std::max(cnt[i], 0), s.M);
      any = any || cnt[i] > 0;
    }
    if (!any) break;
    if (round == FL_MAXROUNDS) {
      // (cannot happen: every flight uses up a hop and an advance has 2 x 4) what is still in flight is LOST, where it left
      for (int i = 0; i < n; i++) {
        auto &s = engines[i]->floats[id];
        if (int rc = floats_mark(engines[i], s, floats_box(s, s.parity).i, cnt[i], FL_LOST)) return rc;
      }
      break;
    }
    for (int i = 0; i < n; i++) {
      hnumo_engine *eng = engines[i];
      auto &s = eng->floats[id];
      HIPCHK(hipSetDevice(eng->device));
      HIPCHK(hipMemsetAsync(floats_box(s, s.parity ^ 1).count, 0, sizeof(int), eng->stream));
      for (size_t k = 0; k < eng->fnb.size(); k++) {
        hnumo_engine *from = engines[eng->fnb[k].rank];
        const int me = floats_nb_index(from, eng->rank);
        if (cnt[from->rank] == 0 || me < 0) continue;
        auto &fs = from->floats[id];
        if (int rc = floats_arrive(eng, s, floats_box(fs, fs.parity), cnt[from->rank], me, (int)k)) return rc;
      }
    }
    for (int i = 0; i < n; i++) engines[i]->floats[id].parity ^= 1;
  }
  int rc = 0;
  for (int i = 0; i < n; i++) {
    hnumo_engine *eng = engines[i];
    HIPCHK(hipSetDevice(eng->device));
    const int r = floats_settle(eng, eng->floats[id], id, who);
    if (!rc) rc = r;
  }
  return rc;
}

// ---- for a host that carries the flight records itself (one engine per process)
extern "C" int hnumo_floats_outbox(hnumo_engine *eng, int32_t id, double *d, int32_t *i, int64_t cap, int64_t *count) {
  const char *who = "hnumo_floats_outbox";
  auto *s = floats_set(eng, id, who);
  if (!s) return HNUMO_ERR_INVALID;
  if (!s->mig) return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the set does not migrate (hnumo_floats_migrate)");
  if (null_arg(eng, count, who, "count")) return HNUMO_ERR_INVALID;
  if (int rc = drain(eng)) return rc;
  const FloatBox b = floats_box(*s, s->parity);
  int n = 0;
  HIPCHK(hipMemcpy(&n, b.count, sizeof(int), hipMemcpyDeviceToHost));
  n = (int)std::min<int64_t>(std::max(n, 0), s->M);
  if (cap < n || (n > 0 && (!d || !i)))
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": d(cap,7), i(cap,6) hold cap = " + std::to_string(cap) +
                                            " records, the outbox has " + std::to_string(n) + " (nothing taken)");
  const size_t M = (size_t)s->M;
  std::vector<double> hd(FL_FD * M);
  std::vector<int32_t> hi(FL_FI * M);
  if (n > 0) {
    for (int v = 0; v < FL_FD; v++) HIPCHK(hipMemcpy(hd.data() + v * M, b.d + v * M, n * sizeof(double), hipMemcpyDeviceToHost));
    for (int v = 0; v < FL_FI; v++) HIPCHK(hipMemcpy(hi.data() + v * M, b.i + v * M, n * sizeof(int), hipMemcpyDeviceToHost));
  }
  // sorted by gid (the order on the device is not deterministic); k leaves as the destination rank
  std::vector<int> ord(n);
  for (int t = 0; t < n; t++) ord[t] = t;
  std::sort(ord.begin(), ord.end(), [&](int a, int c) { return hi[a] < hi[c]; });
  for (int t = 0; t < n; t++) {
    for (int v = 0; v < FL_FD; v++) d[(size_t)v * cap + t] = hd[v * M + ord[t]];
    for (int v = 0; v < FL_FI; v++) i[(size_t)v * cap + t] = hi[v * M + ord[t]];
    const int k = hi[4 * M + ord[t]];
    i[(size_t)4 * cap + t] = k >= 0 && k < (int)eng->fnb.size() ? eng->fnb[k].rank : -1;
  }
  *count = n;
  s->parity ^= 1;
  HIPCHK(hipMemsetAsync(floats_box(*s, s->parity).count, 0, sizeof(int), eng->stream));
  return HNUMO_OK;
}

extern "C" int hnumo_floats_deliver(hnumo_engine *eng, int32_t id, int32_t src_rank, const double *d, const int32_t *i, int64_t cap,
                                    int64_t n) {
  const char *who = "hnumo_floats_deliver";
  auto *s = floats_set(eng, id, who);
  if (!s) return HNUMO_ERR_INVALID;
  if (!s->mig) return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": the set does not migrate (hnumo_floats_migrate)");
  const int from = floats_nb_index(eng, src_rank);
  if (from < 0) return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": rank " + std::to_string(src_rank) + " shares no processor face with this rank");
  if (n < 0 || n > s->M || cap < n || (n > 0 && (!d || !i)))
    return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": n must be in 0..M and <= cap, d(cap,7) and i(cap,6) given");
  for (int64_t t = 0; t < n; t++) {
    const FloatFlight fl{0, 0, 0, 0, 0, 0, 0, i[t], i[cap + t], i[2 * cap + t], i[3 * cap + t], i[4 * cap + t], i[5 * cap + t]};
    if (fl.k == eng->rank && !float_flight_ok(fl, s->M, eng->L, eng->fnb[from].n))
      return fail(eng, HNUMO_ERR_INVALID, std::string(who) + ": record " + std::to_string(t + 1) + " is no flight record (gid, layer, stage, hops or pos out of range)");
  }
  if (n == 0) return HNUMO_OK;
  if (no_state(eng, who)) return HNUMO_ERR_INVALID;
  if (int rc = drain(eng)) return rc;  // (the arrivals of the last delivery read the inbox)
  const FloatBox in = floats_box(*s, 2);
  const size_t M = (size_t)s->M;
  for (int v = 0; v < FL_FD; v++) HIPCHK(hipMemcpy(in.d + v * M, d + (size_t)v * cap, n * sizeof(double), hipMemcpyHostToDevice));
  for (int v = 0; v < FL_FI; v++) HIPCHK(hipMemcpy(in.i + v * M, i + (size_t)v * cap, n * sizeof(int), hipMemcpyHostToDevice));
  // (the flights of these arrivals join the outbox of the current parity, which hnumo_floats_outbox has just emptied)
  s->parity ^= 1;
  const int rc = floats_arrive(eng, *s, in, (int)n, eng->rank, from);
  s->parity ^= 1;
  return rc;
}

extern "C" int hnumo_floats_settle(hnumo_engine *eng, int32_t id) {
  auto *s = floats_set(eng, id, "hnumo_floats_settle");
  if (!s) return HNUMO_ERR_INVALID;
  HIPCHK(hipSetDevice(eng->device));
  return floats_settle(eng, *s, id, "hnumo_floats_settle");
}

// ------------------------------------------------------------------ after a successful step
// Called once run_steps has returned 0 (so a step redone on per-stage launches is observed once), in
// this order: the statistics' sample; the vorticity series' sample; the eddy covariances' sample; the
// energy budget's sample; the region sets' samples; the sample sets' recordings, which see the new sums of a set on the statistics or the covariances; the
// float sets' advance by params.dt, last.  Every
// observer runs whatever the others return (a float cannot skip a step because a series was full);
// the first non-zero code is returned.
static int observers_after_step(hnumo_engine *eng) {
  int rc = 0;
  auto run = [&](int r) {
    if (!rc) rc = r;
  };
  if (eng->stats.on && series_due(eng->stats.series))
    run(stats_sample(eng, "flow statistics after the step (the step itself succeeded)"));
  if (eng->vort.on && eng->vort.series.cap > 0 && series_due(eng->vort.series))
    run(vort_form(eng, true, "vorticity series after the step (the step itself succeeded)"));
  if (eng->cov.on && series_due(eng->cov.series))
    run(cov_sample(eng, "eddy covariances after the step (the step itself succeeded)"));
  if (eng->energy.on && series_due(eng->energy.series))
    run(energy_sample(eng, "energy budget after the step (the step itself succeeded)"));
  if (eng->regions_on)
    for (int id = 0; id < RG_MAXSETS; id++) {
      auto &s = eng->regions[id];
      if (s.used && series_due(s.series)) run(regions_record(eng, s, id, "region series after the step (the step itself succeeded)"));
    }
  for (int id = 0; id < SP_MAXSETS; id++) {
    auto &s = eng->samples[id];
    if (s.used && series_due(s.series)) run(sample_record(eng, s, id, "sample series after the step (the step itself succeeded)"));
  }
  for (int id = 0; id < FL_MAXSETS; id++) {
    auto &s = eng->floats[id];
    // (a migrating set of a grouped engine is advanced by the group, after every engine's observers)
    if (s.used && s.every == 1 && !(s.mig && eng->comm_mode == 1))
      run(floats_advance(eng, s, id, eng->p.dt, "float set after the step (the step itself succeeded)"));
  }
  return rc;
}
