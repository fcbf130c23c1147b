// api.cpp -- the C ABI of include/gsi_hip.h: argument checking, host<->device staging and
// error translation around pipeline.cpp, solvers.cpp and pcga.cpp.  No C++ exception crosses the boundary.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>
#include "../../include/gsi_hip.h"
#include "pcga.hpp"
#include "solvers.hpp"
#include "pointcov.hpp"
#include "fftrf_points.hpp"
#include "cg_state.hpp"
#include "lu_schedule.hpp"

using namespace gsi;

struct gsi_ctx {
  Context c;
};
struct gsi_op {
  Operator op;
};
struct gsi_mat {
  gsi_ctx* ctx;
  Buf buf;
  int64_t rows, cols;
  int refs = 1;            // the caller's handle + one per gsi_basis that points into buf (precision 64: no copy)
};
static void mat_unref(gsi_mat* m) {
  if (m && --m->refs <= 0) delete m;
}
struct gsi_pcgamat {
  gsi_ctx* ctx;
  PcgaLowRank A;
};
struct gsi_precond {
  gsi_ctx* ctx;
  LowRankPrecond pc;
};
struct gsi_basis {
  gsi_ctx* ctx;
  int64_t n, K;
  int precision;          // 64: Z64 points into the gsi_mat; 32: own fp32 copy in buf32
  const double* Z64;
  Buf buf32;
  gsi_mat* owner = nullptr;   // precision 64: the matrix whose buffer Z64 points into, kept alive by this basis
  BasisRef ref() const { return BasisRef{precision == 32 ? (const void*)buf32.p : (const void*)Z64, precision, n, K}; }
};

struct gsi_fwd {
  gsi_ctx* ctx;
  // shared with every OP_FWD_COV operator built on the model (gsi_op_fwd_cov): the last holder frees the resident arrays
  std::shared_ptr<FwdModel> shared = std::make_shared<FwdModel>();
  FwdModel& m = *shared;
};

struct gsi_sampler {
  gsi_ctx* ctx;
  void* plan = nullptr;       // the backend's (Backend::gridcov_sampler_create)
  int ndims;
  int64_t N[3], M[3], n, Mtot;
  double info[4];
  ~gsi_sampler() { if (plan) ctx->c.be->gridcov_sampler_destroy(plan); }
};

namespace {
thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

template <class F>
int guarded(F&& f) {
  try {
    f();
    return GSI_OK;
  } catch (const Error& e) {
    return fail(e.code, e.what());
  } catch (const std::bad_alloc&) {
    return fail(GSI_ERR_OOM, "host allocation failed");
  } catch (const std::exception& e) {
    return fail(GSI_ERR_INTERNAL, e.what());
  } catch (...) {
    return fail(GSI_ERR_INTERNAL, "unknown error");
  }
}

// guarded(f) for the entry points that report which path ran: info_out (may be null) receives {column, path} as f left them,
// also when f threw
template <class F>
int with_info(int64_t* info_out, F&& f) {
  PathInfo info;
  const int st = guarded([&] { f(info); });
  if (info_out) { info_out[0] = info.column; info_out[1] = info.path; }
  return st;
}

// Runs f; if it fails because the backend lost a resource it no longer depends on (Backend::retryable_failure: the
// persistent LU kernel's co-residency on a shared GPU), runs it once more -- the entry points below never modify
// their inputs (operator, Omega, the host panel), so a second run starts from the same state.
template <class F>
void with_retry(Context& c, F&& f) {
  try {
    f();
  } catch (const Error&) {
    // GSI_NO_RETRY: tests of the error path.  With a communicator the ranks must agree on what runs next: no silent re-run
    // (every rank saw the same time-out and has switched paths; the caller repeats the collective call)
    if (!c.be->retryable_failure() || c.comm || getenv("GSI_NO_RETRY") != nullptr) throw;
    c.lu_timeouts_recovered += 1;      // visible in gsi_ctx_path_info: the re-run must not hide that a time-out happened
    f();
  }
}

#define REQUIRE(cond, msg) \
  do { if (!(cond)) throw Error(GSI_ERR_ARG, msg); } while (0)

void check_shard(Context& c, int64_t m, int64_t row0, int64_t mloc) {
  REQUIRE(row0 >= 0 && mloc >= 0 && row0 + mloc <= m, "row shard out of range");
  if (c.nranks() == 1) {
    REQUIRE(row0 == 0 && mloc == m, "single-rank context: the operator must hold all rows");
  } else {
    int64_t r0, ml;
    default_shard(m, c.nranks(), c.rank(), &r0, &ml);
    REQUIRE(r0 == row0 && ml == mloc,
            "multi-rank operators use the block-row layout: pad = ceil(m/nranks), row0 = rank*pad");
  }
}
}  // namespace

extern "C" {

int gsi_version(void) { return GSI_VERSION; }
const char* gsi_last_error(void) { return g_last_error.c_str(); }
const char* gsi_backend_name(void) { return backend_name(); }

int gsi_ctx_create(gsi_ctx** ctx, int device_id) {
  return guarded([&] {
    REQUIRE(ctx != nullptr, "ctx is NULL");
    *ctx = nullptr;
    gsi_ctx* c = new gsi_ctx();
    try {
      c->c.be.reset(make_backend(device_id));
    } catch (...) {
      delete c;
      throw;
    }
    *ctx = c;
  });
}

int gsi_ctx_destroy(gsi_ctx* ctx) {
  return guarded([&] {
    if (!ctx) return;
    ctx->c.comm.reset();
    ctx->c.be.reset();
    delete ctx;
  });
}

int gsi_ctx_sync(gsi_ctx* ctx) {
  return guarded([&] {
    REQUIRE(ctx, "ctx is NULL");
    ctx->c.be->sync();
  });
}

int gsi_comm_unique_id(void* id_out) {
  return guarded([&] {
    REQUIRE(id_out, "id_out is NULL");
    comm_unique_id(id_out);
  });
}

int gsi_ctx_comm_init(gsi_ctx* ctx, int nranks, int rank, const void* id) {
  return guarded([&] {
    REQUIRE(ctx && id, "NULL argument");
    REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "bad rank / nranks");
    REQUIRE(!ctx->c.comm, "communicator already initialised");
    // a 1-rank job needs no communicator; GSI_FORCE_COMM=1 creates one anyway so that the RCCL
    // path (library loading, stream-ordered collectives) can be exercised on a single GPU
    if (nranks == 1 && getenv("GSI_FORCE_COMM") == nullptr) return;
    ctx->c.comm.reset(make_comm(ctx->c.be.get(), nranks, rank, id));
    // how many ranks the communicator really joins: one per rank, summed through it
    Context& c = ctx->c;
    const double one = 1.0;
    double seen = 0.0;
    Buf b(c.be.get(), 1);
    c.be->upload2d(b.p, 1, &one, 1, 1, 1);
    c.comm->allreduce_sum(b.p, 1);
    c.be->download2d(&seen, 1, b.p, 1, 1, 1);
    c.ranks_seen = (int64_t)(seen + 0.5);
    c.be->set_ranks_sharing_device(c.comm->ranks_on_my_device());
    c.comm->ncollectives = 0;
  });
}

int gsi_ctx_host_allgather(gsi_ctx* ctx, const double* mine, int64_t count, double* all_out) {
  return guarded([&] {
    REQUIRE(ctx && mine && all_out && count >= 1, "bad argument");
    Context& c = ctx->c;
    c.be->sync();
    if (!c.comm) {
      std::memcpy(all_out, mine, sizeof(double) * (size_t)count);
      return;
    }
    const int G = c.nranks();
    Buf send(c.be.get(), (size_t)count), recv(c.be.get(), (size_t)count * G);
    c.be->upload2d(send.p, count, mine, count, count, 1);
    const int64_t before = c.comm->ncollectives;
    c.comm->allgather(send.p, recv.p, (size_t)count);
    c.comm->ncollectives = before;          // a host-side barrier / exchange of the caller's is not part of the data path
    c.be->download2d(all_out, count, recv.p, count, count, G);
  });
}

int gsi_ctx_path_info(gsi_ctx* ctx, int64_t* out, int64_t n_out) {
  return guarded([&] {
    REQUIRE(ctx && out && n_out >= 1, "bad argument");
    Context& c = ctx->c;
    int64_t v[GSI_PATH_INFO_COUNT] = {0};
    v[GSI_PATH_LU_FORM_LAST] = c.lu_form_last;
    v[GSI_PATH_LU_SELFTEST_MASK] = c.lus_mr_selftest;
    v[GSI_PATH_COLLECTIVES] = c.comm ? c.comm->ncollectives : 0;
    v[GSI_PATH_RANKS_SEEN] = c.ranks_seen;
    v[GSI_PATH_LU_TIMEOUTS] = c.be->lu_timeouts();
    v[GSI_PATH_LU_TIMEOUTS_RECOVERED] = c.lu_timeouts_recovered;
    for (int f = 0; f < (int)Context::LU_FORMS; ++f) v[GSI_PATH_LU_FORM_COUNTS + f] = c.lu_form_count[f];
    v[GSI_PATH_SVD_CAP_HITS] = c.be->svd_cap_hits();
    v[GSI_PATH_LOWRANK_TAILS] = c.lowrank_tails;
    v[GSI_PATH_LOWRANK_POWER_STEPS] = c.lowrank_power_steps;
    v[GSI_PATH_LOWRANK_POWER_DECLINES] = c.lowrank_power_declines;
    v[GSI_PATH_LOWRANK_SPLIT_LUS] = c.lowrank_split_lus;
    v[GSI_PATH_LOWRANK_SPLIT_DECLINES] = c.lowrank_split_declines;
    v[GSI_PATH_LOWRANK_TAIL_OVERLAPS] = c.be->lowrank_tail_overlaps();
    v[GSI_PATH_LOWRANK_TAIL_SERIES_ROUNDS] = c.be->lowrank_tail_series_rounds();
    for (int64_t i = 0; i < n_out; ++i) out[i] = i < GSI_PATH_INFO_COUNT ? v[i] : 0;
  });
}

int gsi_ctx_pinned_copy_rate(gsi_ctx* ctx, int64_t bytes, double* h2d_gbs, double* d2h_gbs) {
  return guarded([&] {
    REQUIRE(ctx && h2d_gbs && d2h_gbs, "NULL argument");
    REQUIRE(bytes >= 0 && bytes <= ((int64_t)64 << 30), "bad size");
    ctx->c.be->pinned_copy_rate(bytes, h2d_gbs, d2h_gbs);
  });
}

int gsi_ctx_rank(gsi_ctx* ctx, int* rank, int* nranks) {
  return guarded([&] {
    REQUIRE(ctx, "ctx is NULL");
    if (rank) *rank = ctx->c.rank();
    if (nranks) *nranks = ctx->c.nranks();
  });
}

int gsi_op_dense(gsi_ctx* ctx, gsi_op** op, const double* A_rows, int64_t m, int64_t n, int64_t lda,
                 int64_t row0, int64_t m_local) {
  return guarded([&] {
    REQUIRE(ctx && op && A_rows, "NULL argument");
    *op = nullptr;
    REQUIRE(m >= 1 && n >= 1 && lda >= m_local && lda >= 1, "bad matrix shape");
    check_shard(ctx->c, m, row0, m_local);
    std::unique_ptr<gsi_op> o(new gsi_op());
    Operator& A = o->op;
    A.ctx = &ctx->c; A.kind = OP_DENSE; A.m = m; A.n = n; A.row0 = row0; A.mloc = m_local;
    A.ld = m_local > 0 ? ((m_local + 15) / 16) * 16 : 16;   // padded: 16-byte aligned column starts
    A.data = Buf(ctx->c.be.get(), (size_t)A.ld * n);
    ctx->c.be->upload2d(A.data.p, A.ld, A_rows, lda, m_local, n);
    *op = o.release();
  });
}

int gsi_op_lowrank(gsi_ctx* ctx, gsi_op** op, const double* samples, int64_t n, int64_t N, int64_t lds,
                   int center, int64_t row0, int64_t n_local) {
  return guarded([&] {
    REQUIRE(ctx && op && samples, "NULL argument");
    *op = nullptr;
    REQUIRE(n >= 1 && N >= 2 && lds >= n_local && lds >= 1, "bad sample matrix shape (need N >= 2 samples)");
    check_shard(ctx->c, n, row0, n_local);
    std::unique_ptr<gsi_op> o(new gsi_op());
    Operator& A = o->op;
    A.ctx = &ctx->c; A.kind = OP_LOWRANK; A.m = n; A.n = n; A.row0 = row0; A.mloc = n_local; A.N = N;
    A.ld = n_local > 0 ? ((n_local + 15) / 16) * 16 : 16;
    A.data = Buf(ctx->c.be.get(), (size_t)A.ld * N);
    ctx->c.be->upload2d(A.data.p, A.ld, samples, lds, n_local, N);
    if (center) ctx->c.be->center_rows(A.data.p, n_local, N, A.ld);   // lowrank.jl:17-27
    *op = o.release();
  });
}

int gsi_op_lowrank_synthetic(gsi_ctx* ctx, gsi_op** op, int64_t n, int64_t N, uint64_t seed, double decay,
                             int64_t row0, int64_t n_local) {
  return guarded([&] {
    REQUIRE(ctx && op, "NULL argument");
    *op = nullptr;
    REQUIRE(n >= 1 && N >= 2 && decay >= 0.0, "bad synthetic sample parameters (need N >= 2 samples, decay >= 0)");
    check_shard(ctx->c, n, row0, n_local);
    std::unique_ptr<gsi_op> o(new gsi_op());
    Operator& A = o->op;
    A.ctx = &ctx->c; A.kind = OP_LOWRANK; A.m = n; A.n = n; A.row0 = row0; A.mloc = n_local; A.N = N;
    A.ld = n_local > 0 ? ((n_local + 15) / 16) * 16 : 16;
    A.data = Buf(ctx->c.be.get(), (size_t)A.ld * N);
    ctx->c.be->fill_lowrank_samples(A.data.p, A.ld, n_local, N, row0, seed, decay);
    ctx->c.be->center_rows(A.data.p, n_local, N, A.ld);   // lowrank.jl:17-27
    *op = o.release();
  });
}

// The limits of the device sampler (fftrf_sample.hip: a line of at most 8192 points in LDS); -> n, Mtot.  Throws before
// anything is allocated.
static void check_fftrf_grid(int ndims, const int64_t* N, double k0, double dk, double beta, int64_t* n_out, int64_t* mtot_out) {
  REQUIRE(ndims == 2 || ndims == 3, "FFTRF fields: unsupported dimension (ndims must be 2 or 3)");
  REQUIRE(N != nullptr, "N is NULL");
  int64_t n = 1, mtot = 1;
  for (int a = 0; a < ndims; ++a) {
    REQUIRE(N[a] >= 1, "FFTRF fields: grid dimensions must be >= 1");
    const int64_t L = 2 * N[a];
    if ((L & (L - 1)) == 0)
      REQUIRE(N[a] <= 4096, "FFTRF fields: at most 4096 points per axis where 2 N is a power of two (a line of 8192 points)");
    else
      REQUIRE(N[a] <= 2730, "FFTRF fields: at most 2730 points per axis where 2 N is not a power of two (Bluestein's "
                            "convolution of 3 N - 1 points must fit a line of 8192)");
    n *= N[a];
    mtot *= L;
    REQUIRE(mtot < ((int64_t)1 << 31), "FFTRF fields: the doubled grid must have fewer than 2^31 points");
  }
  REQUIRE(n >= 2, "FFTRF fields: a field needs n >= 2 points (the corrected std divides by n - 1)");
  REQUIRE(std::isfinite(k0) && std::isfinite(dk) && std::isfinite(beta), "FFTRF fields: k0, dk and beta must be finite");
  *n_out = n;
  *mtot_out = mtot;
}

int gsi_fftrf_fields(gsi_ctx* ctx, gsi_mat* fields, int ndims, const int64_t* N, double k0, double dk, double beta,
                     const double* phi, int64_t ldphi, uint64_t seed, int64_t field0) {
  return guarded([&] {
    REQUIRE(ctx && fields && fields->ctx == ctx, "bad argument");
    int64_t n = 0, mtot = 0;
    check_fftrf_grid(ndims, N, k0, dk, beta, &n, &mtot);
    REQUIRE(fields->rows == n, "FFTRF fields: the matrix must have n = prod(N) rows");
    REQUIRE(phi == nullptr || ldphi >= mtot, "FFTRF fields: ldphi must be at least Mtot = 2^ndims n");
    REQUIRE(phi != nullptr || field0 >= 0, "FFTRF fields: field0 must be >= 0");
    ctx->c.be->fftrf_fields(fields->buf.p, fields->rows, 0, n, fields->cols, ndims, N, k0, dk, beta, phi, ldphi, seed, field0);
  });
}

int gsi_op_lowrank_fftrf(gsi_ctx* ctx, gsi_op** op, int ndims, const int64_t* N, double k0, double dk, double beta,
                         int64_t numfields, uint64_t seed, int64_t row0, int64_t n_local) {
  return guarded([&] {
    REQUIRE(ctx && op, "NULL argument");
    *op = nullptr;
    int64_t n = 0, mtot = 0;
    check_fftrf_grid(ndims, N, k0, dk, beta, &n, &mtot);
    REQUIRE(numfields >= 2, "LowRankCovMatrix needs numfields >= 2 sample fields");
    check_shard(ctx->c, n, row0, n_local);
    std::unique_ptr<gsi_op> o(new gsi_op());
    Operator& A = o->op;
    A.ctx = &ctx->c; A.kind = OP_LOWRANK; A.m = n; A.n = n; A.row0 = row0; A.mloc = n_local; A.N = numfields;
    A.ld = n_local > 0 ? ((n_local + 15) / 16) * 16 : 16;
    A.data = Buf(ctx->c.be.get(), (size_t)A.ld * numfields);
    // the sampler's normalising write goes straight into the operator's padded buffer
    ctx->c.be->fftrf_fields(A.data.p, A.ld, row0, n_local, numfields, ndims, N, k0, dk, beta, nullptr, 0, seed, 0);
    ctx->c.be->center_rows(A.data.p, n_local, numfields, A.ld);   // lowrank.jl:17-27
    *op = o.release();
  });
}

// The plan of the points [row0, row0 + m_local) on the grid N (fftrf_points.hpp), made before the grid limits of the sampler
// are looked at: refusals become GSI_ERR_ARG before anything is allocated on the device.
static void make_points_plan(int ndims, const int64_t* N, const double* points, int64_t m, const double* box, int64_t row0,
                             int64_t m_local, FftrfPointsPlan* plan) {
  REQUIRE(points != nullptr, "FFTRF points: points is NULL");
  const char* why = fftrf_points_plan(ndims, N, points, m, box, row0, m_local, plan);
  if (why) throw Error(GSI_ERR_ARG, why);
}

int gsi_fftrf_interpolate(gsi_ctx* ctx, gsi_mat* out, const gsi_mat* grid, int ndims, const int64_t* N, const double* points,
                          int64_t m, const double* box, int64_t row0) {
  return guarded([&] {
    REQUIRE(ctx && out && grid && out->ctx == ctx && grid->ctx == ctx, "bad argument");
    FftrfPointsPlan plan;
    make_points_plan(ndims, N, points, m, box, row0, out->rows, &plan);
    int64_t n = 0, mtot = 0;
    check_fftrf_grid(ndims, N, 0.0, 1.0, 0.0, &n, &mtot);
    REQUIRE(grid->rows == n, "FFTRF interpolate: grid must have n = prod(N) rows");
    REQUIRE(out->cols == grid->cols, "FFTRF interpolate: out and grid must have one column per field");
    ctx->c.be->fftrf_interpolate(out->buf.p, out->rows, out->cols, grid->buf.p, grid->rows, plan);
  });
}

int gsi_fftrf_fields_at(gsi_ctx* ctx, gsi_mat* out, int ndims, const int64_t* N, double k0, double dk, double beta,
                        const double* phi, int64_t ldphi, uint64_t seed, int64_t field0, const double* points, int64_t m,
                        const double* box, int64_t row0) {
  return guarded([&] {
    REQUIRE(ctx && out && out->ctx == ctx, "bad argument");
    FftrfPointsPlan plan;
    make_points_plan(ndims, N, points, m, box, row0, out->rows, &plan);
    int64_t n = 0, mtot = 0;
    check_fftrf_grid(ndims, N, k0, dk, beta, &n, &mtot);
    REQUIRE(phi == nullptr || ldphi >= mtot, "FFTRF fields: ldphi must be at least Mtot = 2^ndims n");
    REQUIRE(phi != nullptr || field0 >= 0, "FFTRF fields: field0 must be >= 0");
    ctx->c.be->fftrf_fields_at(out->buf.p, out->rows, out->cols, ndims, N, k0, dk, beta, phi, ldphi, seed, field0, plan);
  });
}

int gsi_op_lowrank_fftrf_at(gsi_ctx* ctx, gsi_op** op, int ndims, const int64_t* N, double k0, double dk, double beta,
                            int64_t numfields, uint64_t seed, const double* points, int64_t m, const double* box,
                            int64_t row0, int64_t m_local) {
  return guarded([&] {
    REQUIRE(ctx && op, "NULL argument");
    *op = nullptr;
    FftrfPointsPlan plan;
    make_points_plan(ndims, N, points, m, box, row0, m_local, &plan);
    int64_t n = 0, mtot = 0;
    check_fftrf_grid(ndims, N, k0, dk, beta, &n, &mtot);
    REQUIRE(numfields >= 2, "LowRankCovMatrix needs numfields >= 2 sample fields");
    check_shard(ctx->c, m, row0, m_local);
    std::unique_ptr<gsi_op> o(new gsi_op());
    Operator& A = o->op;
    A.ctx = &ctx->c; A.kind = OP_LOWRANK; A.m = m; A.n = m; A.row0 = row0; A.mloc = m_local; A.N = numfields;
    A.ld = m_local > 0 ? ((m_local + 15) / 16) * 16 : 16;
    A.data = Buf(ctx->c.be.get(), (size_t)A.ld * numfields);
    ctx->c.be->fftrf_fields_at(A.data.p, A.ld, numfields, ndims, N, k0, dk, beta, nullptr, 0, seed, 0, plan);
    ctx->c.be->center_rows(A.data.p, m_local, numfields, A.ld);   // lowrank.jl:17-27
    *op = o.release();
  });
}

int gsi_op_lowrank_samples(gsi_ctx* ctx, const gsi_op* op, double* samples_out, int64_t ld) {
  return guarded([&] {
    REQUIRE(ctx && op && samples_out, "NULL argument");
    REQUIRE(op->op.ctx == &ctx->c, "operator belongs to another context");
    const Operator& A = op->op;
    REQUIRE(A.kind == OP_LOWRANK, "the operator is not a LowRankCovMatrix");
    REQUIRE(ld >= A.mloc && ld >= 1, "leading dimension too small");
    if (A.mloc > 0) ctx->c.be->download2d(samples_out, ld, A.data.p, A.ld, A.mloc, A.N);
  });
}

int gsi_op_dense_gridcov(gsi_ctx* ctx, gsi_op** op, int64_t nx, int64_t ny, double ell, int kind,
                         int64_t row0, int64_t m_local) {
  return guarded([&] {
    REQUIRE(ctx && op, "NULL argument");
    *op = nullptr;
    REQUIRE(nx >= 1 && ny >= 1 && ell > 0 && (kind == 0 || kind == 1), "bad grid covariance parameters");
    const int64_t n = nx * ny;
    check_shard(ctx->c, n, row0, m_local);
    std::unique_ptr<gsi_op> o(new gsi_op());
    Operator& A = o->op;
    A.ctx = &ctx->c; A.kind = OP_DENSE; A.m = n; A.n = n; A.row0 = row0; A.mloc = m_local;
    A.ld = m_local > 0 ? ((m_local + 15) / 16) * 16 : 16;
    A.data = Buf(ctx->c.be.get(), (size_t)A.ld * n);
    ctx->c.be->fill_gridcov(A.data.p, A.ld, nx, ny, ell, kind, row0, m_local);
    *op = o.release();
  });
}

// table[dx * ny + dy] = k(dx, dy): any stationary kernel on the regular grid
static void make_gridcov_table(gsi_ctx* ctx, gsi_op** op, int64_t nx, int64_t ny, const double* table, int64_t row0,
                               int64_t m_local) {
  REQUIRE(nx >= 1 && ny >= 1, "bad grid");
  REQUIRE(nx * ny < ((int64_t)1 << 31), "implicit grid covariance: more than 2^31 points");
  const int64_t n = nx * ny;
  check_shard(ctx->c, n, row0, m_local);
  std::unique_ptr<gsi_op> o(new gsi_op());
  Operator& A = o->op;
  A.ctx = &ctx->c; A.kind = OP_GRIDCOV_IMPLICIT; A.m = n; A.n = n; A.row0 = row0; A.mloc = m_local;
  A.gx = nx; A.gy = ny; A.ld = 0;
  A.data = Buf(ctx->c.be.get(), (size_t)n);
  ctx->c.be->upload2d(A.data.p, n, table, n, n, 1);
  *op = o.release();
}

int gsi_op_gridcov_implicit_kind(gsi_ctx* ctx, gsi_op** op, int64_t nx, int64_t ny, double ell, int kind, int64_t row0,
                                 int64_t m_local) {
  return guarded([&] {
    REQUIRE(ctx && op, "NULL argument");
    *op = nullptr;
    REQUIRE(nx >= 1 && ny >= 1 && ell > 0 && (kind == 0 || kind == 1),
            "bad grid covariance parameters (kind 0: Gaussian, 1: exponential)");
    std::vector<double> tab((size_t)(nx * ny));
    if (kind == 0) {     // exp(-(dx^2 + dy^2) / (2 ell^2)) as the product of its two 1-D factors
      std::vector<double> ex((size_t)nx), ey((size_t)ny);
      for (int64_t d = 0; d < nx; ++d) ex[(size_t)d] = std::exp(-(double)(d * d) / (2.0 * ell * ell));
      for (int64_t d = 0; d < ny; ++d) ey[(size_t)d] = std::exp(-(double)(d * d) / (2.0 * ell * ell));
      for (int64_t dx = 0; dx < nx; ++dx)
        for (int64_t dy = 0; dy < ny; ++dy) tab[(size_t)(dx * ny + dy)] = ex[(size_t)dx] * ey[(size_t)dy];
    } else {
      for (int64_t dx = 0; dx < nx; ++dx)
        for (int64_t dy = 0; dy < ny; ++dy)
          tab[(size_t)(dx * ny + dy)] = std::exp(-std::sqrt((double)(dx * dx + dy * dy)) / ell);
    }
    make_gridcov_table(ctx, op, nx, ny, tab.data(), row0, m_local);
  });
}

int gsi_op_gridcov_implicit(gsi_ctx* ctx, gsi_op** op, int64_t nx, int64_t ny, double ell, int64_t row0,
                            int64_t m_local) {
  return gsi_op_gridcov_implicit_kind(ctx, op, nx, ny, ell, 0, row0, m_local);
}

int gsi_op_gridcov_implicit_table(gsi_ctx* ctx, gsi_op** op, int64_t nx, int64_t ny, const double* table, int64_t row0,
                                  int64_t m_local) {
  return guarded([&] {
    REQUIRE(ctx && op && table, "NULL argument");
    *op = nullptr;
    make_gridcov_table(ctx, op, nx, ny, table, row0, m_local);
  });
}

int gsi_op_pointcov_implicit(gsi_ctx* ctx, gsi_op** op, const double* points, int64_t n, int d, int kind, double ell,
                             double sigma2, double nugget, int64_t row0, int64_t m_local) {
  return guarded([&] {
    REQUIRE(ctx && op && points, "NULL argument");
    *op = nullptr;
    REQUIRE(n >= 1 && d >= 1 && d <= 3, "point covariance: need n >= 1 points in 1, 2 or 3 dimensions");
    REQUIRE(kind >= 0 && kind < pointcov::NUM_KINDS, "point covariance: kind 0 Gaussian, 1 exponential, 2 Matern 3/2, 3 Matern 5/2");
    REQUIRE(ell > 0.0 && sigma2 > 0.0 && nugget >= 0.0, "point covariance: need ell > 0, sigma2 > 0, nugget >= 0");
    REQUIRE(std::isfinite(ell) && std::isfinite(sigma2) && std::isfinite(nugget), "point covariance: parameters must be finite");
    // The in-loader generator has no clamp in front of its exponential (every vector instruction there is matrix time lost):
    // it saturates to 0 by itself for arguments up to ~1e77 and would return inf / NaN beyond.  The accepted range
    // is checked here instead, once, on the host: finite coordinates within 1e29 correlation lengths of the first point
    // (squared scaled distances <= 3e58 x c1^2: 19 orders of magnitude inside what the generator handles).
    for (int64_t i = 0; i < n; ++i)
      for (int a = 0; a < d; ++a) {
        const double x = points[i * d + a], dx = (x - points[a]) / ell;
        REQUIRE(std::isfinite(x) && std::fabs(dx) <= 1e29,
                "point covariance: coordinates must be finite and within 1e29 correlation lengths of the first point");
      }
    check_shard(ctx->c, n, row0, m_local);
    std::unique_ptr<gsi_op> o(new gsi_op());
    Operator& A = o->op;
    A.ctx = &ctx->c; A.kind = OP_POINTCOV; A.m = n; A.n = n; A.row0 = row0; A.mloc = m_local; A.ld = 0;
    A.pc_d = d; A.pc_kind = kind; A.pc_ell = ell; A.pc_sigma2 = sigma2; A.pc_nugget = nugget;
    A.data = Buf(ctx->c.be.get(), (size_t)n * d);
    ctx->c.be->upload2d(A.data.p, d, points, d, d, n);       // every rank holds all coordinates (8 d n bytes)
    *op = o.release();
  });
}

static void make_fft_powerlaw(gsi_ctx* ctx, gsi_op** op, int ndims, const int64_t* N, double beta, int fftrf) {
  REQUIRE(ctx && op && N, "NULL argument");
  *op = nullptr;
  REQUIRE(ndims >= 1 && ndims <= 3, "fft covariance: 1, 2 or 3 grid dimensions");
  int64_t N3[3] = {1, 1, 1};
  int64_t n = 1;
  for (int a = 0; a < ndims; ++a) {
    REQUIRE(N[a] >= 1, "fft covariance: grid dimensions must be >= 1");
    N3[a] = N[a];
    n *= N[a];
  }
  REQUIRE(n >= 2, "fft covariance: need at least two grid points");
  std::unique_ptr<gsi_op> o(new gsi_op());
  Operator& A = o->op;
  A.ctx = &ctx->c; A.kind = OP_FFT_COV; A.m = n; A.n = n; A.ld = 0;
  // several ranks: every rank holds the plan (spectrum + work array) and transforms ITS columns of a panel; panels are
  // row-sharded between the products (pipeline.cpp: rows_to_cols / cols_to_rows), so row0 / mloc = the block-row layout
  default_shard(n, ctx->c.nranks(), ctx->c.rank(), &A.row0, &A.mloc);
  A.fft_ndims = ndims;
  for (int a = 0; a < 3; ++a) A.fft_N[a] = N3[a];
  own_fft_plan(A, ctx->c.be->fftcov_create(N3, beta, fftrf));
  *op = o.release();
}

int gsi_op_fft_powerlaw(gsi_ctx* ctx, gsi_op** op, int ndims, const int64_t* N, double beta) {
  return guarded([&] { make_fft_powerlaw(ctx, op, ndims, N, beta, 0); });
}

int gsi_op_fft_powerlaw_fftrf(gsi_ctx* ctx, gsi_op** op, int ndims, const int64_t* N, double beta) {
  return guarded([&] { make_fft_powerlaw(ctx, op, ndims, N, beta, 1); });
}

// The FFT operator for a covariance function (kind / ell / theta / sigma2) or a table of lags (table / table_mirror) on the
// grid: OP_FFT_COV with another plan (Backend::fftcov_create_lags).  The arguments are checked here; the limit on the embedded
// points (2^31) is the backend's, as for the power-law plans: refused before it allocates anything.
enum { NOT_A_DERIVATIVE = -1000 };     // make_fft_gridcov's dparam for the covariance itself (any other value is checked)
static void make_fft_gridcov(gsi_ctx* ctx, gsi_op** op, int ndims, const int64_t* N, int kind, const double* ell, double theta,
                             double sigma2, double nugget, const double* table, const double* table_mirror, bool from_table,
                             int dparam = NOT_A_DERIVATIVE) {
  REQUIRE(ctx && op && N, "NULL argument");
  *op = nullptr;
  REQUIRE(ndims >= 1 && ndims <= 3, "fft covariance: 1, 2 or 3 grid dimensions");
  int64_t N3[3] = {1, 1, 1};
  int64_t n = 1;
  for (int a = 0; a < ndims; ++a) {
    REQUIRE(N[a] >= 1, "fft covariance: grid dimensions must be >= 1");
    // (the backend's limit and message, repeated here because the tables below are read with n = prod N[a] entries first)
    REQUIRE(N[a] <= 4096, "fft covariance: at most 4096 grid points per axis (a line must fit LDS)");
    N3[a] = N[a];
    n *= N[a];
  }
  REQUIRE(n >= 2, "fft covariance: need at least two grid points");
  REQUIRE(std::isfinite(nugget) && nugget >= 0.0, "fft grid covariance: nugget must be finite and >= 0");
  double ell3[3] = {1.0, 1.0, 1.0};
  if (from_table) {
    REQUIRE(table, "fft grid covariance: table is NULL");
    REQUIRE(table_mirror == nullptr || ndims == 2, "fft grid covariance: table_mirror is for 2-D grids only");
    for (int64_t e = 0; e < n; ++e) REQUIRE(std::isfinite(table[e]), "fft grid covariance: table entries must be finite");
    if (table_mirror) {
      for (int64_t e = 0; e < n; ++e)
        REQUIRE(std::isfinite(table_mirror[e]), "fft grid covariance: table_mirror entries must be finite");
      // c(t0, -t1) = c(t0, t1) where t0 == 0 (central symmetry) or t1 == 0 (the same lag)
      auto agree = [](double a, double b) { return std::fabs(a - b) <= 1e-12 * std::max(std::fabs(a), std::fabs(b)); };
      for (int64_t t0 = 0; t0 < N3[0]; ++t0)
        REQUIRE(agree(table[t0], table_mirror[t0]), "fft grid covariance: table_mirror must agree with table where t1 == 0");
      for (int64_t t1 = 0; t1 < N3[1]; ++t1)
        REQUIRE(agree(table[t1 * N3[0]], table_mirror[t1 * N3[0]]),
                "fft grid covariance: table_mirror must agree with table where t0 == 0 (c(-t) = c(t))");
    }
  } else {
    REQUIRE(kind >= 0 && kind < pointcov::NUM_KINDS, "fft grid covariance: kind 0 Gaussian, 1 exponential, 2 Matern 3/2, 3 Matern 5/2");
    REQUIRE(ell, "fft grid covariance: ell is NULL");
    for (int a = 0; a < ndims; ++a) {
      REQUIRE(std::isfinite(ell[a]) && ell[a] > 0.0, "fft grid covariance: every ell[a] must be finite and > 0");
      ell3[a] = ell[a];
    }
    REQUIRE(std::isfinite(sigma2) && sigma2 > 0.0, "fft grid covariance: sigma2 must be finite and > 0");
    REQUIRE(std::isfinite(theta), "fft grid covariance: theta must be finite");
    REQUIRE(theta == 0.0 || ndims == 2, "fft grid covariance: theta (a rotation) is for 2-D grids only");
    if (dparam != NOT_A_DERIVATIVE) {
      REQUIRE(dparam >= 0 && dparam < pointcov::NUM_DPARAMS,
              "fft grid covariance derivative: param must be one of GSI_DPARAM_LOG_SIGMA2 .. GSI_DPARAM_NUGGET (0 .. 6)");
      REQUIRE(dparam != pointcov::D_THETA || ndims == 2, "fft grid covariance derivative: GSI_DPARAM_THETA is for 2-D grids only");
      REQUIRE(dparam < pointcov::D_LOG_ELL0 || dparam > pointcov::D_LOG_ELL2 || dparam - pointcov::D_LOG_ELL0 < ndims,
              "fft grid covariance derivative: GSI_DPARAM_LOG_ELL<a> needs a < ndims");
    }
  }
  std::unique_ptr<gsi_op> o(new gsi_op());
  Operator& A = o->op;
  A.ctx = &ctx->c; A.kind = OP_FFT_COV; A.m = n; A.n = n; A.ld = 0;
  default_shard(n, ctx->c.nranks(), ctx->c.rank(), &A.row0, &A.mloc);     // as make_fft_powerlaw: the plan is replicated
  A.fft_ndims = ndims;
  for (int a = 0; a < 3; ++a) A.fft_N[a] = N3[a];
  if (dparam != NOT_A_DERIVATIVE) own_fft_plan(A, ctx->c.be->fftcov_create_lags_deriv(N3, kind, ell3, theta, sigma2, dparam));
  else own_fft_plan(A, ctx->c.be->fftcov_create_lags(N3, kind, ell3, theta, sigma2, nugget, table, table_mirror));
  *op = o.release();
}

// A = W C W' (OP_FFT_COV_AT): C = grid_op's covariance, whose plan is shared, W = the interpolation of
// gsi_fftrf_interpolate at the m points on grid_op's own grid.  The points plan and its inverted index go to the device here
// and stay there.
int gsi_op_fft_at(gsi_ctx* ctx, gsi_op** op, const gsi_op* grid_op, const double* points, int64_t m, const double* box) {
  return guarded([&] {
    REQUIRE(ctx && op && grid_op, "NULL argument");
    *op = nullptr;
    const Operator& C = grid_op->op;
    REQUIRE(C.ctx == &ctx->c, "gsi_op_fft_at: the grid operator belongs to another context");
    REQUIRE(C.kind == OP_FFT_COV && C.plan != nullptr,
            "gsi_op_fft_at: the grid operator must be an FFT covariance operator (gsi_op_fft_powerlaw[_fftrf], gsi_op_fft_gridcov[_table])");
    REQUIRE(!ctx->c.comm, "gsi_op_fft_at: one GPU only -- not available on a context with a communicator");
    REQUIRE(C.fft_ndims == 2 || C.fft_ndims == 3, "gsi_op_fft_at: the grid operator must have 2 or 3 axes (a 1-D grid is not supported)");
    FftrfPointsPlan plan;
    make_points_plan(C.fft_ndims, C.fft_N, points, m, box, 0, m, &plan);     // refuses an axis of fewer than 2 points, bad points
    std::unique_ptr<gsi_op> o(new gsi_op());
    Operator& A = o->op;
    A.ctx = &ctx->c; A.kind = OP_FFT_COV_AT; A.m = m; A.n = m; A.row0 = 0; A.mloc = m; A.ld = 0;
    A.fft_ndims = C.fft_ndims;
    for (int a = 0; a < 3; ++a) A.fft_N[a] = C.fft_N[a];
    A.plan = C.plan;
    A.plan_ref = C.plan_ref;
    own_points_at(A, ctx->c.be->points_at_create(plan, A.at_info));
    *op = o.release();
  });
}

// A = W C' W' on the points of an existing OP_FFT_COV_AT operator: the points plan and its inverted index are
// shared (Operator::at_ref), nothing is planned or uploaded.  A fit builds its operators anew at every parameter value.
int gsi_op_fft_at_like(gsi_ctx* ctx, gsi_op** op, const gsi_op* grid_op, const gsi_op* like) {
  return guarded([&] {
    REQUIRE(ctx && op && grid_op && like, "NULL argument");
    *op = nullptr;
    const Operator& C = grid_op->op;
    const Operator& B = like->op;
    REQUIRE(C.ctx == &ctx->c, "gsi_op_fft_at_like: the grid operator belongs to another context");
    REQUIRE(B.ctx == &ctx->c, "gsi_op_fft_at_like: the like operator belongs to another context");
    REQUIRE(C.kind == OP_FFT_COV && C.plan != nullptr,
            "gsi_op_fft_at_like: the grid operator must be an FFT covariance operator (gsi_op_fft_powerlaw[_fftrf], gsi_op_fft_gridcov[_table], gsi_op_fft_gridcov_deriv)");
    REQUIRE(B.kind == OP_FFT_COV_AT && B.at != nullptr, "gsi_op_fft_at_like: like must be an operator of gsi_op_fft_at");
    REQUIRE(!ctx->c.comm, "gsi_op_fft_at_like: one GPU only -- not available on a context with a communicator");
    REQUIRE(C.fft_ndims == B.fft_ndims && C.fft_N[0] == B.fft_N[0] && C.fft_N[1] == B.fft_N[1] && C.fft_N[2] == B.fft_N[2],
            "gsi_op_fft_at_like: the grid operator and the like operator must have the same grid shape");
    std::unique_ptr<gsi_op> o(new gsi_op());
    Operator& A = o->op;
    A.ctx = &ctx->c; A.kind = OP_FFT_COV_AT; A.m = B.m; A.n = B.m; A.row0 = 0; A.mloc = B.m; A.ld = 0;
    A.fft_ndims = C.fft_ndims;
    for (int a = 0; a < 3; ++a) A.fft_N[a] = C.fft_N[a];
    A.plan = C.plan;
    A.plan_ref = C.plan_ref;
    A.at = B.at;
    A.at_ref = B.at_ref;
    for (int k = 0; k < 4; ++k) A.at_info[k] = B.at_info[k];
    *op = o.release();
  });
}

int gsi_fftrf_spread(gsi_ctx* ctx, gsi_mat* grid_out, const gsi_mat* in, int ndims, const int64_t* N, const double* points,
                     int64_t m, const double* box, int64_t row0) {
  return guarded([&] {
    REQUIRE(ctx && grid_out && in && grid_out->ctx == ctx && in->ctx == ctx, "bad argument");
    REQUIRE(grid_out != in, "FFTRF spread: grid_out and in must be different matrices");
    FftrfPointsPlan plan;
    make_points_plan(ndims, N, points, m, box, row0, in->rows, &plan);
    int64_t n = 0, mtot = 0;
    check_fftrf_grid(ndims, N, 0.0, 1.0, 0.0, &n, &mtot);
    REQUIRE(grid_out->rows == n, "FFTRF spread: grid_out must have n = prod(N) rows");
    REQUIRE(grid_out->cols == in->cols, "FFTRF spread: grid_out and in must have one column per field");
    Backend* be = ctx->c.be.get();
    void* at = be->points_at_create(plan, nullptr);
    try {
      be->points_at_spread(at, grid_out->buf.p, grid_out->rows, grid_out->cols, in->buf.p, in->rows);
    } catch (...) {
      be->points_at_destroy(at);
      throw;
    }
    be->points_at_destroy(at);      // (release is ordered on the stream: the kernels above still see the plan)
  });
}

int gsi_op_fft_gridcov(gsi_ctx* ctx, gsi_op** op, int ndims, const int64_t* N, int kind, const double* ell, double theta,
                       double sigma2, double nugget) {
  return guarded([&] { make_fft_gridcov(ctx, op, ndims, N, kind, ell, theta, sigma2, nugget, nullptr, nullptr, false); });
}

int gsi_op_fft_gridcov_table(gsi_ctx* ctx, gsi_op** op, int ndims, const int64_t* N, const double* table,
                             const double* table_mirror, double nugget) {
  return guarded([&] { make_fft_gridcov(ctx, op, ndims, N, 0, nullptr, 0.0, 1.0, nugget, table, table_mirror, true); });
}

// d C / d param for the covariance of gsi_op_fft_gridcov: the same checks, then the derivative's plan
int gsi_op_fft_gridcov_deriv(gsi_ctx* ctx, gsi_op** op, int ndims, const int64_t* N, int kind, const double* ell, double theta,
                             double sigma2, int param) {
  return guarded([&] {
    if (op) *op = nullptr;
    REQUIRE(param >= 0 && param < pointcov::NUM_DPARAMS,
            "fft grid covariance derivative: param must be one of GSI_DPARAM_LOG_SIGMA2 .. GSI_DPARAM_NUGGET (0 .. 6)");
    make_fft_gridcov(ctx, op, ndims, N, kind, ell, theta, sigma2, 0.0, nullptr, nullptr, false, param);
  });
}

// ---- Gaussian fields with a grid covariance function (circulant embedding; Backend::gridcov_sampler_*) ----
int gsi_gridcov_sampler_create(gsi_ctx* ctx, gsi_sampler** sampler, int ndims, const int64_t* N, const int64_t* embed, int kind,
                               const double* ell, double theta, double sigma2, double nugget, double neg_tol, double* info) {
  double inf4[4] = {NAN, NAN, NAN, NAN};
  const int st = guarded([&] {
    REQUIRE(ctx && sampler, "gridcov sampler: ctx or sampler is NULL");
    *sampler = nullptr;
    REQUIRE(ndims == 2 || ndims == 3, "gridcov sampler: ndims must be 2 or 3");
    REQUIRE(N != nullptr, "gridcov sampler: N is NULL");
    std::unique_ptr<gsi_sampler> s(new gsi_sampler());
    s->ctx = ctx; s->ndims = ndims; s->n = 1; s->Mtot = 1;
    for (int a = 0; a < 3; ++a) { s->N[a] = 1; s->M[a] = 1; }
    for (int a = 0; a < ndims; ++a) {
      REQUIRE(N[a] >= 1, "gridcov sampler: every N[a] must be >= 1");
      // (before the default embedding is formed: 2 N[a] must not overflow, and no torus holds more than 4096 box points)
      REQUIRE(N[a] <= 4096, "gridcov sampler: N[a] must be <= 4096 (the torus needs embed[a] >= 2 N[a], and embed[a] <= 8192)");
      s->N[a] = N[a];
      s->n *= N[a];
    }
    REQUIRE(s->n >= 2, "gridcov sampler: a field needs n = prod(N) >= 2 points");
    for (int a = 0; a < ndims; ++a) {
      int64_t M = 2;
      while (M < 2 * N[a]) M <<= 1;                    // the operator's embedding (fft_embed_size)
      if (embed) M = embed[a];
      REQUIRE(M >= 1 && (M & (M - 1)) == 0, "gridcov sampler: every embed[a] must be a power of two");
      REQUIRE(M >= 2 * N[a], "gridcov sampler: every embed[a] must be >= 2 N[a]");
      REQUIRE(M <= 8192, "gridcov sampler: every embed[a] must be <= 8192 (a line must fit LDS)");
      s->M[a] = M;
      s->Mtot *= M;
      REQUIRE(s->Mtot < ((int64_t)1 << 31), "gridcov sampler: Mtot = prod(embed) must be < 2^31");
    }
    REQUIRE(kind >= 0 && kind < pointcov::NUM_KINDS, "gridcov sampler: kind 0 Gaussian, 1 exponential, 2 Matern 3/2, 3 Matern 5/2");
    REQUIRE(ell, "gridcov sampler: ell is NULL");
    double ell3[3] = {1.0, 1.0, 1.0};
    for (int a = 0; a < ndims; ++a) {
      REQUIRE(std::isfinite(ell[a]) && ell[a] > 0.0, "gridcov sampler: every ell[a] must be finite and > 0");
      ell3[a] = ell[a];
    }
    REQUIRE(std::isfinite(sigma2) && sigma2 > 0.0, "gridcov sampler: sigma2 must be finite and > 0");
    REQUIRE(std::isfinite(nugget) && nugget >= 0.0, "gridcov sampler: nugget must be finite and >= 0");
    REQUIRE(std::isfinite(theta), "gridcov sampler: theta must be finite");
    REQUIRE(theta == 0.0 || ndims == 2, "gridcov sampler: theta (a rotation) is for 2-D grids only");
    REQUIRE(neg_tol >= 0.0 && neg_tol <= 1.0, "gridcov sampler: neg_tol must be in [0, 1]");      // (NaN fails both)
    // with a communicator every rank builds the plan: fields are generated whole and each rank keeps its rows
    s->plan = ctx->c.be->gridcov_sampler_create(ndims, s->N, s->M, kind, ell3, theta, sigma2, nugget, neg_tol, inf4);
    for (int i = 0; i < 4; ++i) s->info[i] = inf4[i];
    *sampler = s.release();
  });
  if (info) for (int i = 0; i < 4; ++i) info[i] = inf4[i];           // also when the plan was refused (GSI_ERR_NOT_POSDEF)
  return st;
}

int gsi_gridcov_sampler_info(const gsi_sampler* sampler, int64_t* M, double* info) {
  return guarded([&] {
    REQUIRE(sampler, "gridcov sampler: sampler is NULL");
    if (M) for (int a = 0; a < 3; ++a) M[a] = sampler->M[a];
    if (info) for (int i = 0; i < 4; ++i) info[i] = sampler->info[i];
  });
}

int gsi_gridcov_sampler_spectrum(gsi_ctx* ctx, const gsi_sampler* sampler, double* lam_out) {
  return guarded([&] {
    REQUIRE(ctx && sampler && sampler->ctx == ctx, "gridcov sampler: ctx or sampler is NULL, or the sampler belongs to another context");
    REQUIRE(lam_out, "gridcov sampler: lam_out is NULL");
    ctx->c.be->gridcov_sampler_spectrum(sampler->plan, lam_out);
  });
}

int gsi_gridcov_sampler_destroy(gsi_sampler* sampler) {
  return guarded([&] { delete sampler; });
}

int gsi_gridcov_fields(gsi_ctx* ctx, const gsi_sampler* sampler, gsi_mat* fields, const double* eps, int64_t ldeps, uint64_t seed,
                       int64_t field0) {
  return guarded([&] {
    REQUIRE(ctx && sampler && sampler->ctx == ctx, "gridcov fields: ctx or sampler is NULL, or the sampler belongs to another context");
    REQUIRE(fields && fields->ctx == ctx, "gridcov fields: fields is NULL or belongs to another context");
    REQUIRE(fields->rows == sampler->n, "gridcov fields: fields must have n = prod(N) rows");
    REQUIRE(eps == nullptr || ldeps >= sampler->Mtot, "gridcov fields: ldeps must be at least Mtot = prod(embed)");
    REQUIRE(eps != nullptr || (field0 >= 0 && field0 % 2 == 0), "gridcov fields: field0 must be even and >= 0 (a pair is one transform)");
    ctx->c.be->gridcov_sampler_fields(sampler->plan, fields->buf.p, fields->rows, 0, sampler->n, fields->cols, eps, ldeps, seed,
                                      field0);
  });
}

int gsi_op_lowrank_gridcov(gsi_ctx* ctx, gsi_op** op, const gsi_sampler* sampler, int64_t numfields, uint64_t seed, int64_t row0,
                           int64_t n_local) {
  return guarded([&] {
    REQUIRE(ctx && op, "NULL argument");
    *op = nullptr;
    REQUIRE(sampler && sampler->ctx == ctx, "gridcov fields: sampler is NULL or belongs to another context");
    REQUIRE(numfields >= 2, "LowRankCovMatrix needs numfields >= 2 sample fields");
    const int64_t n = sampler->n;
    check_shard(ctx->c, n, row0, n_local);
    std::unique_ptr<gsi_op> o(new gsi_op());
    Operator& A = o->op;
    A.ctx = &ctx->c; A.kind = OP_LOWRANK; A.m = n; A.n = n; A.row0 = row0; A.mloc = n_local; A.N = numfields;
    A.ld = n_local > 0 ? ((n_local + 15) / 16) * 16 : 16;
    A.data = Buf(ctx->c.be.get(), (size_t)A.ld * numfields);
    // the sampler's last pass writes straight into the operator's padded buffer
    ctx->c.be->gridcov_sampler_fields(sampler->plan, A.data.p, A.ld, row0, n_local, numfields, nullptr, 0, seed, 0);
    ctx->c.be->center_rows(A.data.p, n_local, numfields, A.ld);   // lowrank.jl:17-27
    *op = o.release();
  });
}

int gsi_op_destroy(gsi_op* op) {
  return guarded([&] { delete op; });
}

int gsi_op_size(const gsi_op* op, int64_t* m, int64_t* n, int64_t* row0, int64_t* m_local) {
  return guarded([&] {
    REQUIRE(op, "op is NULL");
    if (m) *m = op->op.m;
    if (n) *n = op->op.n;
    if (row0) *row0 = op->op.row0;
    if (m_local) *m_local = op->op.mloc;
  });
}

int gsi_op_mul(gsi_ctx* ctx, const gsi_op* op, int trans, const double* X, int64_t ldx, int64_t l, double* Y,
               int64_t ldy) {
  return guarded([&] {
    REQUIRE(ctx && op && X && Y, "NULL argument");
    REQUIRE(op->op.ctx == &ctx->c, "operator belongs to another context");
    const Operator& A = op->op;
    Backend* be = ctx->c.be.get();
    REQUIRE(l >= 1, "need at least one column");
    const int64_t rows_in = trans ? A.m : A.n, rows_out = trans ? A.n : A.m;
    REQUIRE(ldx >= rows_in && ldy >= rows_out, "leading dimension too small");
    Buf Xd(be, (size_t)rows_in * l), Yd(be, (size_t)rows_out * l);
    be->upload2d(Xd.p, rows_in, X, ldx, rows_in, l);
    if (!trans) {
      Buf Yloc(be, (size_t)(A.mloc > 0 ? A.mloc : 1) * l);
      op_mul(A, Xd.p, A.n, l, Yloc.p, A.mloc);
      gather_rows(ctx->c, A, Yloc.p, A.mloc, l, Yd.p);
    } else {
      op_mul_t(A, Xd.p + A.row0, A.m, l, Yd.p, A.n);
    }
    be->download2d(Y, ldy, Yd.p, rows_out, rows_out, l);
    check_async_errors(ctx->c);
  });
}

int gsi_rangefinder(gsi_ctx* ctx, const gsi_op* op, const double* Omega, int64_t l, int64_t numiterations,
                    double* Q_out) {
  return guarded([&] {
    REQUIRE(ctx && op && Omega && Q_out, "NULL argument");
    REQUIRE(op->op.ctx == &ctx->c, "operator belongs to another context");
    const Operator& A = op->op;
    Backend* be = ctx->c.be.get();
    REQUIRE(l >= 1, "l must be positive");
    Buf Om(be, (size_t)A.n * l);
    be->upload2d(Om.p, A.n, Omega, A.n, A.n, l);
    with_retry(ctx->c, [&] {
      Buf Qloc = rangefinder(A, Om.p, l, numiterations);
      Buf Qfull(be, (size_t)A.m * l);
      gather_rows(ctx->c, A, Qloc.p, A.mloc, l, Qfull.p);
      check_async_errors(ctx->c);
      be->download2d(Q_out, A.m, Qfull.p, A.m, A.m, l);
    });
  });
}

int gsi_randsvd(gsi_ctx* ctx, const gsi_op* op, const double* Omega, int64_t K, int64_t p, int64_t q,
                double* Z_out, double* S_out) {
  return guarded([&] {
    REQUIRE(ctx && op && Omega && Z_out, "NULL argument");
    REQUIRE(op->op.ctx == &ctx->c, "operator belongs to another context");
    REQUIRE(K >= 0 && p >= 0 && K + p >= 1, "need K >= 0, p >= 0, K + p >= 1");
    const Operator& A = op->op;
    Backend* be = ctx->c.be.get();
    const int64_t l = K + p;
    Buf Om(be, (size_t)A.n * l), Z(be, (size_t)A.n * l), S(be, (size_t)l);
    be->upload2d(Om.p, A.n, Omega, A.n, A.n, l);
    with_retry(ctx->c, [&] {
      randsvd(A, Om.p, K, p, q, Z.p, S.p);
      check_async_errors(ctx->c);
    });
    be->download2d(Z_out, A.n, Z.p, A.n, A.n, l);
    if (S_out) be->download2d(S_out, l, S.p, l, l, 1);
  });
}

// ---- the dense operator still in HOST memory: what getxis(Q::Matrix, ...) is called with ----------------------------
}  // extern "C" (the helpers below are C++)
namespace {
// A dense operator whose rows are on their way: allocated, the upload started in row blocks (single rank, large matrices;
// otherwise uploaded synchronously), `pending_upload` set for the first product.  The guard ends the transfer on every path.
struct UploadGuard {
  Backend* be = nullptr;
  void* h = nullptr;
  ~UploadGuard() {
    if (!h) return;
    try { be->upload2d_end(h); } catch (...) {}
  }
};
std::unique_ptr<gsi_op> dense_op_streaming(gsi_ctx* ctx, const double* A_host, int64_t m, int64_t n, int64_t lda, UploadGuard& g) {
  REQUIRE(m >= 1 && n >= 1 && lda >= m, "bad matrix shape");
  REQUIRE(ctx->c.nranks() == 1, "the host-matrix entry points are single-rank: with a communicator upload this rank's rows with gsi_op_dense");
  std::unique_ptr<gsi_op> o(new gsi_op());
  Operator& A = o->op;
  Backend* be = ctx->c.be.get();
  A.ctx = &ctx->c; A.kind = OP_DENSE; A.m = m; A.n = n; A.row0 = 0; A.mloc = m;
  A.ld = ((m + 15) / 16) * 16;
  A.data = Buf(be, (size_t)A.ld * n);
  const int64_t mb = be->upload_block_rows(m, n);
  g.be = be;
  g.h = be->upload2d_begin(A.data.p, A.ld, A_host, lda, m, n, mb);
  if (g.h != nullptr) { A.pending_upload = g.h; A.pending_block_rows = mb; }
  return o;
}
}  // namespace
extern "C" {

int gsi_randsvd_dense_host(gsi_ctx* ctx, const double* A_host, int64_t m, int64_t n, int64_t lda, const double* Omega,
                           int64_t K, int64_t p, int64_t q, double* Z_out, double* S_out, gsi_op** op_out) {
  return guarded([&] {
    REQUIRE(ctx && A_host && Omega && Z_out, "NULL argument");
    if (op_out) *op_out = nullptr;
    REQUIRE(K >= 0 && p >= 0 && K + p >= 1, "need K >= 0, p >= 0, K + p >= 1");
    Backend* be = ctx->c.be.get();
    const int64_t l = K + p;
    REQUIRE(m >= 1 && n >= 1 && lda >= m, "bad matrix shape");
    Buf Om(be, (size_t)n * l), Z(be, (size_t)n * l), S(be, (size_t)l);
    be->upload2d(Om.p, n, Omega, n, n, l);                  // Omega first: the first block's product needs all of it
    std::unique_ptr<gsi_op> o;                              // (declared before the guard: the transfer ends before the buffer goes)
    UploadGuard g;
    o = dense_op_streaming(ctx, A_host, m, n, lda, g);
    const Operator& A = o->op;
    with_retry(ctx->c, [&] {
      randsvd(A, Om.p, K, p, q, Z.p, S.p);
      check_async_errors(ctx->c);
    });
    be->download2d(Z_out, n, Z.p, n, n, l);
    if (S_out) be->download2d(S_out, l, S.p, l, l, 1);
    if (op_out) *op_out = o.release();
  });
}

int gsi_rangefinder_dense_host(gsi_ctx* ctx, const double* A_host, int64_t m, int64_t n, int64_t lda, const double* Omega,
                               int64_t l, int64_t numiterations, double* Q_out, gsi_op** op_out) {
  return guarded([&] {
    REQUIRE(ctx && A_host && Omega && Q_out, "NULL argument");
    if (op_out) *op_out = nullptr;
    REQUIRE(l >= 1, "l must be positive");
    REQUIRE(m >= 1 && n >= 1 && lda >= m, "bad matrix shape");
    Backend* be = ctx->c.be.get();
    Buf Om(be, (size_t)n * l);
    be->upload2d(Om.p, n, Omega, n, n, l);
    std::unique_ptr<gsi_op> o;                              // (declared before the guard: the transfer ends before the buffer goes)
    UploadGuard g;
    o = dense_op_streaming(ctx, A_host, m, n, lda, g);
    const Operator& A = o->op;
    with_retry(ctx->c, [&] {
      Buf Q = rangefinder(A, Om.p, l, numiterations);
      check_async_errors(ctx->c);
      be->download2d(Q_out, m, Q.p, m, m, l);
    });
    if (op_out) *op_out = o.release();
  });
}

int gsi_eig_nystrom(gsi_ctx* ctx, const gsi_op* op, const double* Q, int64_t j, double* U_out,
                    double* Sigma_out) {
  return guarded([&] {
    REQUIRE(ctx && op && Q && U_out && Sigma_out, "NULL argument");
    REQUIRE(op->op.ctx == &ctx->c, "operator belongs to another context");
    const Operator& A = op->op;
    Backend* be = ctx->c.be.get();
    REQUIRE(j >= 1 && j <= A.n, "bad number of columns in Q");
    Buf Qd(be, (size_t)A.n * j), U(be, (size_t)A.m * j), S(be, (size_t)j);
    be->upload2d(Qd.p, A.n, Q, A.n, A.n, j);
    eig_nystrom(A, Qd.p, j, U.p, S.p);
    be->download2d(U_out, A.m, U.p, A.m, A.m, j);
    be->download2d(Sigma_out, j, S.p, j, j, 1);
    check_async_errors(ctx->c);
  });
}

int gsi_rangefinder_adaptive(gsi_ctx* ctx, const gsi_op* op, gsi_randn_fn randn, void* user, double epsilon,
                             int64_t r, double* Q_out, int64_t* ncols_out) {
  return guarded([&] {
    REQUIRE(ctx && op && randn && Q_out && ncols_out, "NULL argument");
    REQUIRE(op->op.ctx == &ctx->c, "operator belongs to another context");
    *ncols_out = rangefinder_adaptive(op->op, randn, user, epsilon, r, Q_out);
    check_async_errors(ctx->c);
  });
}

// ---- device-resident matrices ------------------------------------------------------
int gsi_mat_create(gsi_ctx* ctx, gsi_mat** mat, int64_t rows, int64_t cols) {
  return guarded([&] {
    REQUIRE(ctx && mat, "NULL argument");
    *mat = nullptr;
    REQUIRE(rows >= 1 && cols >= 1, "bad shape");
    std::unique_ptr<gsi_mat> m(new gsi_mat());
    m->ctx = ctx; m->rows = rows; m->cols = cols;
    m->buf = Buf(ctx->c.be.get(), (size_t)rows * cols);
    *mat = m.release();
  });
}
int gsi_mat_destroy(gsi_mat* mat) {
  return guarded([&] { mat_unref(mat); });     // the buffer lives on while a 64-bit gsi_basis still points into it
}
int gsi_mat_upload(gsi_ctx* ctx, gsi_mat* mat, const double* host, int64_t ldh) {
  return guarded([&] {
    REQUIRE(ctx && mat && host && mat->ctx == ctx, "bad argument");
    REQUIRE(ldh >= mat->rows, "leading dimension too small");
    ctx->c.be->upload2d(mat->buf.p, mat->rows, host, ldh, mat->rows, mat->cols);
  });
}
int gsi_mat_download(gsi_ctx* ctx, const gsi_mat* mat, double* host, int64_t ldh) {
  return guarded([&] {
    REQUIRE(ctx && mat && host && mat->ctx == ctx, "bad argument");
    REQUIRE(ldh >= mat->rows, "leading dimension too small");
    ctx->c.be->download2d(host, ldh, mat->buf.p, mat->rows, mat->rows, mat->cols);
  });
}
int gsi_mat_randn(gsi_ctx* ctx, gsi_mat* mat, uint64_t seed) {
  return guarded([&] {
    REQUIRE(ctx && mat && mat->ctx == ctx, "bad argument");
    ctx->c.be->randn(mat->buf.p, (size_t)mat->rows * mat->cols, seed);
  });
}

int gsi_op_mul_dev(gsi_ctx* ctx, const gsi_op* op, int trans, const gsi_mat* X, gsi_mat* Y) {
  return guarded([&] {
    REQUIRE(ctx && op && X && Y, "NULL argument");
    REQUIRE(op->op.ctx == &ctx->c && X->ctx == ctx && Y->ctx == ctx, "objects belong to another context");
    const Operator& A = op->op;
    const int64_t l = X->cols;
    const int64_t rows_in = trans ? A.m : A.n, rows_out = trans ? A.n : A.m;
    REQUIRE(X->rows == rows_in && Y->rows == rows_out && Y->cols == l, "shape mismatch");
    if (!trans) {
      if (ctx->c.nranks() == 1) {
        op_mul(A, X->buf.p, A.n, l, Y->buf.p, A.m);
      } else {
        Buf Yloc(ctx->c.be.get(), (size_t)(A.mloc > 0 ? A.mloc : 1) * l);
        op_mul(A, X->buf.p, A.n, l, Yloc.p, A.mloc);
        gather_rows(ctx->c, A, Yloc.p, A.mloc, l, Y->buf.p);
      }
    } else {
      op_mul_t(A, X->buf.p + A.row0, A.m, l, Y->buf.p, A.n);
    }
  });
}

int gsi_rangefinder_dev(gsi_ctx* ctx, const gsi_op* op, const gsi_mat* Omega, int64_t numiterations,
                        gsi_mat* Q) {
  return guarded([&] {
    REQUIRE(ctx && op && Omega && Q, "NULL argument");
    REQUIRE(op->op.ctx == &ctx->c && Omega->ctx == ctx && Q->ctx == ctx, "objects belong to another context");
    const Operator& A = op->op;
    const int64_t l = Omega->cols;
    REQUIRE(Omega->rows == A.n, "Omega must have size(A,2) rows");
    REQUIRE(Q->rows == A.m && Q->cols == l, "Q must be size(A,1) x l");
    with_retry(ctx->c, [&] {
      Buf Qloc = rangefinder(A, Omega->buf.p, l, numiterations);
      gather_rows(ctx->c, A, Qloc.p, A.mloc, l, Q->buf.p);
      check_async_errors(ctx->c);
    });
  });
}

int gsi_randsvd_dev(gsi_ctx* ctx, const gsi_op* op, const gsi_mat* Omega, int64_t K, int64_t p, int64_t q,
                    gsi_mat* Z, gsi_mat* S) {
  return guarded([&] {
    REQUIRE(ctx && op && Omega && Z, "NULL argument");
    REQUIRE(op->op.ctx == &ctx->c && Omega->ctx == ctx && Z->ctx == ctx, "objects belong to another context");
    REQUIRE(K >= 0 && p >= 0 && K + p >= 1, "need K >= 0, p >= 0, K + p >= 1");
    const Operator& A = op->op;
    const int64_t l = K + p;
    REQUIRE(Omega->rows == A.n && Omega->cols == l, "Omega must be size(A,2) x (K+p)");
    REQUIRE(Z->rows == A.n && Z->cols == l, "Z must be size(A,2) x (K+p)");
    Backend* be = ctx->c.be.get();
    Buf Stmp;
    double* Sp;
    if (S) {
      REQUIRE(S->ctx == ctx && S->rows * S->cols == l, "S must hold K+p values");
      Sp = S->buf.p;
    } else {
      Stmp = Buf(be, (size_t)l);
      Sp = Stmp.p;
    }
    with_retry(ctx->c, [&] {
      randsvd(A, Omega->buf.p, K, p, q, Z->buf.p, Sp);
      check_async_errors(ctx->c);
    });
  });
}

int gsi_randsvd_rows(gsi_ctx* ctx, const gsi_op* op, const gsi_mat* Omega_rows, int64_t K, int64_t p, int64_t q,
                     gsi_mat* Z_rows, gsi_mat* S) {
  return guarded([&] {
    REQUIRE(ctx && op && Omega_rows && Z_rows, "NULL argument");
    REQUIRE(op->op.ctx == &ctx->c && Omega_rows->ctx == ctx && Z_rows->ctx == ctx, "objects belong to another context");
    REQUIRE(K >= 0 && p >= 0 && K + p >= 1, "need K >= 0, p >= 0, K + p >= 1");
    const Operator& A = op->op;
    const int64_t l = K + p;
    int64_t r0, nloc;
    default_shard(A.n, ctx->c.nranks(), ctx->c.rank(), &r0, &nloc);
    REQUIRE(nloc >= 1, "this rank holds no rows of the panel");
    REQUIRE(Omega_rows->rows == nloc && Omega_rows->cols == l, "Omega_rows must be (this rank's rows of size(A,2)) x (K+p)");
    REQUIRE(Z_rows->rows == nloc && Z_rows->cols == l, "Z_rows must be (this rank's rows of size(A,2)) x (K+p)");
    Backend* be = ctx->c.be.get();
    Buf Stmp;
    double* Sp;
    if (S) {
      REQUIRE(S->ctx == ctx && S->rows * S->cols == l, "S must hold K+p values");
      Sp = S->buf.p;
    } else {
      Stmp = Buf(be, (size_t)l);
      Sp = Stmp.p;
    }
    with_retry(ctx->c, [&] {
      randsvd_rows(A, Omega_rows->buf.p, K, p, q, Z_rows->buf.p, Sp);
      check_async_errors(ctx->c);
    });
  });
}

// ---- panel primitives ----------------------------------------------------------------
int gsi_lu_L(gsi_ctx* ctx, const double* Y, int64_t m, int64_t l, double* L_out, int32_t* ipiv_out) {
  return guarded([&] {
    REQUIRE(ctx && Y && L_out, "NULL argument");
    REQUIRE(m >= 1 && l >= 1 && l <= m, "lu_L: need 1 <= l <= m (tall panel)");
    Backend* be = ctx->c.be.get();
    Buf P(be, (size_t)m * l);
    with_retry(ctx->c, [&] {
      be->upload2d(P.p, m, Y, m, m, l);
      be->lu_L(P.p, m, l, m, ipiv_out);
      check_async_errors(ctx->c);
    });
    be->download2d(L_out, m, P.p, m, m, l);
  });
}

int gsi_lu_schedule(int64_t l, int32_t* widths, int32_t* nblocks) {
  return guarded([&] {
    REQUIRE(widths && nblocks, "NULL argument");
    REQUIRE(l >= 1, "lu_schedule: need l >= 1");
    std::vector<int> w;
    REQUIRE(lu_schedule_choose(l, w), "lu_schedule: GSI_LU_SCHEDULE is not a list of block widths (16, 32, 48, 64; a last block of 1 .. 64)");
    for (size_t i = 0; i < w.size(); ++i) widths[i] = w[i];
    *nblocks = (int32_t)w.size();
  });
}

int gsi_lu_L_dev(gsi_ctx* ctx, gsi_mat* Y, int32_t* ipiv_out) {
  return guarded([&] {
    REQUIRE(ctx && Y, "NULL argument");
    REQUIRE(Y->ctx == ctx, "matrix belongs to another context");
    REQUIRE(Y->rows >= 1 && Y->cols >= 1 && Y->cols <= Y->rows, "lu_L: need 1 <= l <= m (tall panel)");
    Backend* be = ctx->c.be.get();
    {
      ScopedPhase ph(be, PH_LU);
      be->lu_L(Y->buf.p, Y->rows, Y->cols, Y->rows, ipiv_out);     // in place: a lost co-residency leaves no input to re-run from
    }
    check_async_errors(ctx->c);
  });
}

int gsi_lu_L_sharded(gsi_ctx* ctx, const double* Y, int64_t m, int64_t l, double* L_out, int32_t* ipiv_out) {
  return guarded([&] {
    REQUIRE(ctx && Y && L_out, "NULL argument");
    REQUIRE(m >= 1 && l >= 1 && l <= m, "lu_L: need 1 <= l <= m (tall panel)");
    Context& c = ctx->c;
    Backend* be = c.be.get();
    int64_t r0, ml;
    default_shard(m, c.nranks(), c.rank(), &r0, &ml);
    int64_t r00, ml0;
    default_shard(m, c.nranks(), 0, &r00, &ml0);
    REQUIRE(l <= ml0, "sharded lu: the first rank must hold the first l rows (l <= ceil(m / nranks))");
    Buf P(be, (size_t)std::max<int64_t>(ml, 1) * l);
    if (ml > 0) be->upload2d(P.p, ml, Y + r0, m, ml, l);
    lu_panel_sharded(c, P.p, m, r0, ml, l);
    Buf Full(be, (size_t)m * l);
    Operator shape;
    shape.m = m; shape.row0 = r0; shape.mloc = ml;
    gather_rows(c, shape, P.p, std::max<int64_t>(ml, 1), l, Full.p);
    be->download2d(L_out, m, Full.p, m, m, l);
    if (ipiv_out) be->lus_pivots(ipiv_out, l);
    check_async_errors(c);
  });
}

int gsi_lu_L_sharded_virtual(gsi_ctx* ctx, const double* Y, int64_t m, int64_t l, int nshards, double* L_out,
                             int32_t* ipiv_out) {
  return guarded([&] {
    REQUIRE(ctx && Y && L_out, "NULL argument");
    REQUIRE(m >= 1 && l >= 1 && l <= m, "lu_L: need 1 <= l <= m (tall panel)");
    REQUIRE(nshards >= 1 && nshards <= 64, "need 1 <= nshards <= 64");
    REQUIRE(nshards == 1 || l <= (m + nshards - 1) / nshards,
            "sharded lu: the first shard must hold the first l rows (l <= ceil(m / nshards))");
    Context& c = ctx->c;
    Backend* be = c.be.get();
    std::vector<Buf> shards;
    std::vector<double*> ptrs;
    for (int g = 0; g < nshards; ++g) {
      int64_t r0, ml;
      default_shard(m, nshards, g, &r0, &ml);
      shards.emplace_back(be, (size_t)std::max<int64_t>(ml, 1) * l);
      if (ml > 0) be->upload2d(shards.back().p, ml, Y + r0, m, ml, l);
      ptrs.push_back(shards.back().p);
    }
    lu_panel_sharded_virtual(c, ptrs.data(), m, l, nshards);
    check_async_errors(c);
    for (int g = 0; g < nshards; ++g) {
      int64_t r0, ml;
      default_shard(m, nshards, g, &r0, &ml);
      if (ml > 0) be->download2d(L_out + r0, m, ptrs[(size_t)g], ml, ml, l);
    }
    if (ipiv_out) be->lus_pivots(ipiv_out, l);
  });
}

int gsi_qr_thinQ(gsi_ctx* ctx, const double* Y, int64_t m, int64_t l, double* Q_out, double* R_out) {
  return guarded([&] {
    REQUIRE(ctx && Y && Q_out, "NULL argument");
    REQUIRE(m >= 1 && l >= 1 && l <= m, "qr_thinQ: need 1 <= l <= m (tall panel)");
    Backend* be = ctx->c.be.get();
    Buf P(be, (size_t)m * l), R(be, (size_t)l * l);
    be->upload2d(P.p, m, Y, m, m, l);
    {
      ScopedPhase ph(be, PH_QR);
      be->qr_thinQ(P.p, m, l, m, R.p);
    }
    be->download2d(Q_out, m, P.p, m, m, l);
    if (R_out) be->download2d(R_out, l, R.p, l, l, l);
    check_async_errors(ctx->c);
  });
}

int gsi_svd_tall(gsi_ctx* ctx, const double* W, int64_t n, int64_t l, double* V_out, double* S_out) {
  return guarded([&] {
    REQUIRE(ctx && W && V_out && S_out, "NULL argument");
    REQUIRE(n >= 1 && l >= 1 && l <= n, "svd_tall: need 1 <= l <= n");
    Backend* be = ctx->c.be.get();
    Buf Wd(be, (size_t)n * l), V(be, (size_t)n * l), S(be, (size_t)l);
    be->upload2d(Wd.p, n, W, n, n, l);
    svd_tall(ctx->c, Wd.p, n, l, -1, V.p, S.p);
    be->download2d(V_out, n, V.p, n, n, l);
    be->download2d(S_out, l, S.p, l, l, 1);
    check_async_errors(ctx->c);
  });
}

int gsi_gemm(gsi_ctx* ctx, int trans, int64_t m, int64_t l, int64_t k, double alpha, const double* A,
             int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc) {
  return guarded([&] {
    REQUIRE(ctx && A && B && C, "NULL argument");
    REQUIRE(m >= 1 && l >= 1 && k >= 1, "bad shape");
    const int64_t ar = trans ? k : m, ac = trans ? m : k;
    REQUIRE(lda >= ar && ldb >= k && ldc >= m, "leading dimension too small");
    Backend* be = ctx->c.be.get();
    Buf Ad(be, (size_t)ar * ac), Bd(be, (size_t)k * l), Cd(be, (size_t)m * l);
    be->upload2d(Ad.p, ar, A, lda, ar, ac);
    be->upload2d(Bd.p, k, B, ldb, k, l);
    if (trans) be->gemm_tn(m, l, k, alpha, Ad.p, ar, Bd.p, k, 0.0, Cd.p, m);
    else be->gemm_nn(m, l, k, alpha, Ad.p, ar, Bd.p, k, 0.0, Cd.p, m);
    be->download2d(C, ldc, Cd.p, m, m, l);
    check_async_errors(ctx->c);
  });
}

int gsi_gemm_view(gsi_ctx* ctx, int form, int trans, int64_t m, int64_t l, int64_t k, double alpha, double beta,
                  const double* A, int64_t lda, int64_t a_off, const double* B, int64_t ldb, int64_t b_off, double* C,
                  int64_t ldc, int64_t c_off, int64_t m_full, int64_t r0, int64_t* plan_out) {
  return guarded([&] {
    REQUIRE(ctx && A && C && plan_out, "NULL argument");
    REQUIRE(form >= 0 && form <= 3, "gemm_view: form is 0 (gemm), 1 (syrk upper), 2 (trmm upper) or 3 (NN row block)");
    REQUIRE(m >= 1 && l >= 1 && k >= 1, "bad shape");
    REQUIRE(form == 1 || B, "NULL argument");
    REQUIRE(form == 0 || (alpha == 1.0 && beta == 0.0), "gemm_view: forms 1 to 3 compute C = op(A) B (alpha 1, beta 0)");
    REQUIRE(form == 0 || !trans, "gemm_view: trans belongs to form 0");
    REQUIRE(form != 1 || m == l, "gemm_view: form 1 is the l x l product A'A (m == l)");
    REQUIRE(form != 3 || (r0 >= 0 && r0 + m <= m_full), "gemm_view: row block outside the full product");
    // the operands as they lie on the device: A ar x ac, B k x l, C crows x l
    const bool tn = trans || form == 1;
    const int64_t ar = (form == 3) ? m_full : (tn ? k : m), ac = tn ? m : k;
    const int64_t crows = (form == 3) ? m_full : m;
    REQUIRE(lda >= ar && ldc >= crows && (form == 1 || ldb >= k), "leading dimension too small");
    REQUIRE(a_off >= 0 && b_off >= 0 && c_off >= 0, "negative offset");
    Backend* be = ctx->c.be.get();
    const size_t na = (size_t)a_off + (size_t)lda * (size_t)ac, nc = (size_t)c_off + (size_t)ldc * (size_t)l;
    const size_t nb = (form == 1) ? 1 : (size_t)b_off + (size_t)ldb * (size_t)l;
    Buf Ad(be, na), Bd(be, nb), Cd(be, nc);
    // whatever the views do not cover is NaN (all bytes 0xFF): a read of the padding poisons the result
    be->fill_bytes(Ad.p, 0xFF, na);
    be->fill_bytes(Bd.p, 0xFF, nb);
    be->upload2d(Ad.p + a_off, lda, A, ar, ar, ac);
    if (form != 1) be->upload2d(Bd.p + b_off, ldb, B, k, k, l);
    be->upload2d(Cd.p, (int64_t)nc, C, (int64_t)nc, (int64_t)nc, 1);          // C: the whole image, there and back
    be->gemm_view(form, trans != 0, m, l, k, alpha, Ad.p + a_off, lda, Bd.p + b_off, ldb, beta, Cd.p + c_off, ldc, m_full, r0,
                  plan_out);
    be->download2d(C, (int64_t)nc, Cd.p, (int64_t)nc, (int64_t)nc, 1);
    check_async_errors(ctx->c);
  });
}

int gsi_cq_gram_round(gsi_ctx* ctx, int64_t l, int check, const double* gram, double* R, double* X, int32_t* flag_out,
                      int32_t* series_out, double* norm_out) {
  return guarded([&] {
    REQUIRE(ctx && gram && R && X && flag_out && series_out && norm_out, "NULL argument");
    REQUIRE(l >= 1 && l <= 384, "cq_gram_round: 1 <= l <= 384");
    Backend* be = ctx->c.be.get();
    Buf Gd(be, (size_t)l * l), Xd(be, (size_t)l * l);
    be->fill_bytes(Xd.p, 0xFF, (size_t)l * l);                // (NaN: X has to be written whole)
    be->upload2d(Gd.p, l, gram, l, l, l);
    int32_t out2[2] = {0, 0};
    be->cq_gram_round_view(Gd.p, l, Xd.p, check != 0, out2, norm_out);
    be->download2d(R, l, Gd.p, l, l, l);
    be->download2d(X, l, Xd.p, l, l, l);
    *flag_out = out2[0];
    *series_out = out2[1];
    check_async_errors(ctx->c);
  });
}

// ---- consumers -----------------------------------------------------------------------
int gsi_pcga_params(gsi_ctx* ctx, const double* Z, int64_t n, int64_t K, const double* s, const double* X,
                    double delta, double* out) {
  return guarded([&] {
    REQUIRE(ctx && Z && s && X && out, "NULL argument");
    REQUIRE(n >= 1 && K >= 1, "bad shape");
    Buf Zd(ctx->c.be.get(), (size_t)n * K);
    ctx->c.be->upload2d(Zd.p, n, Z, n, n, K);
    basis_params(ctx->c, BasisRef{Zd.p, 64, n, K}, s, X, delta, out);
  });
}

int gsi_pcga_update(gsi_ctx* ctx, const double* Z, int64_t n, int64_t K, const double* X, double beta_bar,
                    const double* etas, int64_t nobs, const double* xi_bar, double* s_out) {
  return guarded([&] {
    REQUIRE(ctx && Z && X && etas && xi_bar && s_out, "NULL argument");
    REQUIRE(n >= 1 && K >= 1 && nobs >= 1, "bad shape");
    Buf Zd(ctx->c.be.get(), (size_t)n * K);
    ctx->c.be->upload2d(Zd.p, n, Z, n, n, K);
    basis_update(ctx->c, BasisRef{Zd.p, 64, n, K}, X, beta_bar, etas, nobs, xi_bar, s_out);
  });
}

int gsi_pcga_params_dev(gsi_ctx* ctx, const gsi_mat* basis, int64_t K, const double* s, const double* X,
                        double delta, double* out) {
  return guarded([&] {
    REQUIRE(ctx && basis && s && X && out, "NULL argument");
    REQUIRE(basis->ctx == ctx && K >= 1 && K <= basis->cols, "bad basis / K");
    basis_params(ctx->c, BasisRef{basis->buf.p, 64, basis->rows, K}, s, X, delta, out);
  });
}

int gsi_pcga_update_dev(gsi_ctx* ctx, const gsi_mat* basis, int64_t K, const double* X, double beta_bar,
                        const double* etas, int64_t nobs, const double* xi_bar, double* s_out) {
  return guarded([&] {
    REQUIRE(ctx && basis && X && etas && xi_bar && s_out, "NULL argument");
    REQUIRE(basis->ctx == ctx && K >= 1 && K <= basis->cols && nobs >= 1, "bad basis / K / nobs");
    basis_update(ctx->c, BasisRef{basis->buf.p, 64, basis->rows, K}, X, beta_bar, etas, nobs, xi_bar, s_out);
  });
}

int gsi_mat_download_col(gsi_ctx* ctx, const gsi_mat* mat, int64_t col, double* host) {
  return guarded([&] {
    REQUIRE(ctx && mat && host && mat->ctx == ctx, "bad argument");
    REQUIRE(col >= 0 && col < mat->cols, "column out of range");
    ctx->c.be->download2d(host, mat->rows, mat->buf.p + (size_t)col * mat->rows, mat->rows, mat->rows, 1);
  });
}

// ---- LSQR consumers ------------------------------------------------------------------
int gsi_op_lowrank_solve(gsi_ctx* ctx, const gsi_op* op, const double* b, double* x_out, int64_t* iters_out) {
  return guarded([&] {
    REQUIRE(ctx && op && b && x_out, "NULL argument");
    REQUIRE(op->op.ctx == &ctx->c, "operator belongs to another context");
    const Operator& A = op->op;
    Backend* be = ctx->c.be.get();
    Buf bd(be, (size_t)A.n), xd(be, (size_t)A.n);
    be->upload2d(bd.p, A.n, b, A.n, A.n, 1);
    const int64_t it = lowrank_solve(A, bd.p, xd.p);
    be->download2d(x_out, A.n, xd.p, A.n, A.n, 1);
    if (iters_out) *iters_out = it;
    check_async_errors(ctx->c);
  });
}

// ---- kriging systems: block CG on any operator ------------------------------------------
//      plain (gsi_op_solve_cg, gsi_op_solve), preconditioned (gsi_op_solve_pcg, gsi_op_solve_pcg_host)
//      and traced (gsi_op_solve_trace; section 4.6k).  info has 4, 6 and 7 entries for the three: INFO_* below, and nothing
//      here writes beyond the length an entry point passes.
namespace {
enum { INFO_CG = 4, INFO_PCG = 6, INFO_TRACE = 7 };
// the checks that need no memory; info is cleared first.  pc may be null unless need_pc.
void check_solve_args(gsi_ctx* ctx, const gsi_op* op, const double* diag, const gsi_precond* pc, bool need_pc, int64_t b,
                      double tol, int64_t maxiter, int64_t* info, int ninfo) {
  if (info) for (int i = 0; i < ninfo; ++i) info[i] = 0;
  REQUIRE(ctx && op, "gsi_op_solve: ctx or op is NULL");
  REQUIRE(op->op.ctx == &ctx->c, "gsi_op_solve: op belongs to another context");
  block_cg_check(op->op, nullptr, b, tol, maxiter);
  if (diag)
    for (int64_t i = 0; i < op->op.n; ++i)
      if (!(diag[i] >= 0.0 && diag[i] <= 1.79769313486231570815e308))
        throw Error(GSI_ERR_ARG, "gsi_op_solve: diag[" + std::to_string(i) + "] is negative or not finite");
  REQUIRE(pc || !need_pc, "gsi_op_solve_pcg: pc is NULL");
  if (pc) {
    REQUIRE(pc->ctx == ctx, "gsi_op_solve_pcg: pc belongs to another context");
    block_cg_check(op->op, &pc->pc, b, tol, maxiter);          // (what it refuses about pc: the rest has passed above)
  }
}
// B and X of the entry points that take resident panels
void check_resident_panels(const std::string& fn, gsi_ctx* ctx, const Operator& A, const gsi_mat* B, const gsi_mat* X) {
  REQUIRE(B->ctx == ctx && X->ctx == ctx, fn + ": B or X belongs to another context");
  REQUIRE(B->rows == A.n, fn + ": B must have size(A, 1) rows");
  REQUIRE(X->rows == A.n && X->cols == B->cols, fn + ": X must have the shape of B");
  REQUIRE(X != B && X->buf.p != B->buf.p, fn + ": X must not be B");
}
// the upload of diag, the solve on resident panels, and the report: info (ninfo entries; the seventh needs a trace), relres
// and iters are filled before a breakdown is raised.  who: how the message of a breakdown begins.
void solve_resident(const char* who, gsi_ctx* ctx, const Operator& A, const double* diag, const gsi_precond* pc, const double* Bd,
                    double* Xd, int64_t b, double tol, int64_t maxiter, int64_t* info, int ninfo, double* relres, int64_t* iters,
                    CgTrace* trace) {
  Backend* be = ctx->c.be.get();
  Buf dd;
  if (diag) {
    dd = Buf(be, (size_t)A.n);
    be->upload2d(dd.p, A.n, diag, A.n, A.n, 1);
  }
  const BlockCgInfo r = block_cg(A, diag ? dd.p : nullptr, pc ? &pc->pc : nullptr, Bd, Xd, b, tol, maxiter, relres, iters, trace);
  if (info) {
    const int64_t v[INFO_TRACE] = {r.products, r.converged, r.path, r.breakdown_column, r.breakdown_kind, r.K,
                                   trace ? trace->truncated : 0};
    for (int i = 0; i < ninfo; ++i) info[i] = v[i];
  }
  check_async_errors(ctx->c);
  if (r.breakdown_column != 0)
    throw Error(GSI_ERR_NOT_POSDEF, std::string(who) + ": " +
                                        (r.breakdown_kind == 2 ? "r'z is not positive and finite (the preconditioner is not positive definite)"
                                                               : "A + diag is not positive definite along the search direction") +
                                        " of column " + std::to_string(r.breakdown_column));
}
// the entry points that stage B and X through the host: fn names the entry point in what it refuses
int solve_staged(const std::string& fn, const char* who, gsi_ctx* ctx, const gsi_op* op, const double* diag, const gsi_precond* pc,
                 bool need_pc, const double* B, int64_t ldb, int64_t b, double* X, int64_t ldx, double tol, int64_t maxiter,
                 int64_t* info, int ninfo, double* relres, int64_t* iters) {
  return guarded([&] {
    REQUIRE(B && X, fn + ": B or X is NULL");
    check_solve_args(ctx, op, diag, pc, need_pc, b, tol, maxiter, info, ninfo);
    const Operator& A = op->op;
    REQUIRE(ldb >= A.n, fn + ": ldb is smaller than size(A, 1), the rows of B");
    REQUIRE(ldx >= A.n, fn + ": ldx is smaller than size(A, 1), the rows of X");
    REQUIRE(X != B, fn + ": X must not be B");
    Backend* be = ctx->c.be.get();
    Buf Bd(be, (size_t)A.n * b), Xd(be, (size_t)A.n * b);
    be->upload2d(Bd.p, A.n, B, ldb, A.n, b);
    // (the solution comes back also when the solve broke down: what the columns had reached)
    try {
      solve_resident(who, ctx, A, diag, pc, Bd.p, Xd.p, b, tol, maxiter, info, ninfo, relres, iters, nullptr);
    } catch (const Error& e) {
      if (e.code == GSI_ERR_NOT_POSDEF) be->download2d(X, ldx, Xd.p, A.n, A.n, b);
      throw;
    }
    be->download2d(X, ldx, Xd.p, A.n, A.n, b);
  });
}
// ... and the ones whose B and X are resident
int solve_mats(const std::string& fn, const char* who, gsi_ctx* ctx, const gsi_op* op, const double* diag, const gsi_precond* pc,
               bool need_pc, const gsi_mat* B, gsi_mat* X, double tol, int64_t maxiter, int64_t* info, int ninfo, double* relres,
               int64_t* iters) {
  return guarded([&] {
    REQUIRE(B && X, fn + ": B or X is NULL");
    check_solve_args(ctx, op, diag, pc, need_pc, B->cols, tol, maxiter, info, ninfo);
    check_resident_panels(fn, ctx, op->op, B, X);
    solve_resident(who, ctx, op->op, diag, pc, B->buf.p, X->buf.p, B->cols, tol, maxiter, info, ninfo, relres, iters, nullptr);
  });
}
}  // namespace

int gsi_op_solve_cg(gsi_ctx* ctx, const gsi_op* op, const double* diag, const gsi_mat* B, gsi_mat* X, double tol,
                    int64_t maxiter, int64_t* info, double* relres, int64_t* iters) {
  return solve_mats("gsi_op_solve_cg", "conjugate gradients", ctx, op, diag, nullptr, false, B, X, tol, maxiter, info, INFO_CG,
                    relres, iters);
}

int gsi_op_solve(gsi_ctx* ctx, const gsi_op* op, const double* diag, const double* B, int64_t ldb, int64_t b, double* X,
                 int64_t ldx, double tol, int64_t maxiter, int64_t* info, double* relres, int64_t* iters) {
  return solve_staged("gsi_op_solve", "conjugate gradients", ctx, op, diag, nullptr, false, B, ldb, b, X, ldx, tol, maxiter, info,
                      INFO_CG, relres, iters);
}

// ---- the low-rank-plus-diagonal preconditioner and the preconditioned solve ----
int gsi_precond_lowrank_create(gsi_ctx* ctx, gsi_precond** pc, const gsi_mat* Z, int64_t K, const double* diag, double shift,
                               double* info_out) {
  return guarded([&] {
    REQUIRE(ctx && pc && Z, "gsi_precond_lowrank_create: ctx, pc or Z is NULL");
    *pc = nullptr;
    if (info_out) info_out[0] = info_out[1] = info_out[2] = info_out[3] = 0.0;
    REQUIRE(Z->ctx == ctx, "gsi_precond_lowrank_create: Z belongs to another context");
    double lo = 0.0, hi = 0.0;
    precond_lowrank_check(ctx->c, Z->rows, Z->cols, K, diag, shift, &lo, &hi);
    std::unique_ptr<gsi_precond> h(new gsi_precond());
    h->ctx = ctx;
    precond_lowrank_build(h->pc, ctx->c, Z->buf.p, Z->rows, K, diag, shift);
    if (info_out) { info_out[0] = (double)K; info_out[1] = (double)Z->rows; info_out[2] = lo; info_out[3] = hi; }
    *pc = h.release();
  });
}
int gsi_precond_destroy(gsi_precond* pc) {
  return guarded([&] { delete pc; });
}
int gsi_precond_info(const gsi_precond* pc, double* info_out) {
  return guarded([&] {
    REQUIRE(pc && info_out, "gsi_precond_info: NULL argument");
    info_out[0] = (double)pc->pc.K; info_out[1] = (double)pc->pc.n; info_out[2] = pc->pc.dmin; info_out[3] = pc->pc.dmax;
  });
}
int gsi_precond_apply(gsi_ctx* ctx, const gsi_precond* pc, const gsi_mat* R, gsi_mat* Zout) {
  return guarded([&] {
    REQUIRE(ctx && pc && R && Zout, "gsi_precond_apply: NULL argument");
    REQUIRE(pc->ctx == ctx, "gsi_precond_apply: pc belongs to another context");
    REQUIRE(R->ctx == ctx && Zout->ctx == ctx, "gsi_precond_apply: R or Zout belongs to another context");
    REQUIRE(R->rows == pc->pc.n && R->cols >= 1, "gsi_precond_apply: R must have the preconditioner's rows");
    REQUIRE(Zout->rows == R->rows && Zout->cols == R->cols, "gsi_precond_apply: Zout must have the shape of R");
    REQUIRE(Zout != R && Zout->buf.p != R->buf.p, "gsi_precond_apply: Zout must not be R");
    precond_apply(pc->pc, R->buf.p, R->cols, Zout->buf.p);
    check_async_errors(ctx->c);
  });
}

int gsi_op_solve_pcg(gsi_ctx* ctx, const gsi_op* op, const double* diag, const gsi_precond* pc, const gsi_mat* B, gsi_mat* X,
                     double tol, int64_t maxiter, int64_t* info, double* relres, int64_t* iters) {
  return solve_mats("gsi_op_solve_pcg", "preconditioned conjugate gradients", ctx, op, diag, pc, true, B, X, tol, maxiter, info,
                    INFO_PCG, relres, iters);
}

int gsi_op_solve_pcg_host(gsi_ctx* ctx, const gsi_op* op, const double* diag, const gsi_precond* pc, const double* B,
                          int64_t ldb, int64_t b, double* X, int64_t ldx, double tol, int64_t maxiter, int64_t* info,
                          double* relres, int64_t* iters) {
  return solve_staged("gsi_op_solve_pcg_host", "preconditioned conjugate gradients", ctx, op, diag, pc, true, B, ldb, b, X, ldx,
                      tol, maxiter, info, INFO_PCG, relres, iters);
}

// ---- log-determinants by stochastic Lanczos quadrature: the traced solve, the quadrature alone, draws of N(0, P) and
//      log det P ----
int gsi_op_solve_trace(gsi_ctx* ctx, const gsi_op* op, const double* diag, const gsi_precond* pc, const gsi_mat* B, gsi_mat* X,
                       int64_t nquad, int64_t qmax, double tol, int64_t maxiter, int64_t* info, double* relres, int64_t* iters,
                       double* quad_out) {
  return guarded([&] {
    if (info) for (int i = 0; i < 7; ++i) info[i] = 0;
    REQUIRE(B && X, "gsi_op_solve_trace: B or X is NULL");
    const int64_t b = B->cols;
    if (quad_out) for (int64_t j = 0; j < 2 * b; ++j) quad_out[j] = 0.0;
    check_solve_args(ctx, op, diag, pc, false, b, tol, maxiter, info, INFO_TRACE);
    check_resident_panels("gsi_op_solve_trace", ctx, op->op, B, X);
    REQUIRE(qmax >= 1, "gsi_op_solve_trace: qmax must be at least 1");
    REQUIRE(qmax <= 4096, "gsi_op_solve_trace: qmax exceeds 4096");
    REQUIRE(nquad >= 0 && nquad <= b, "gsi_op_solve_trace: nquad must lie in 0 .. the columns of B");
    Backend* be = ctx->c.be.get();
    CgTrace trace;
    trace.qmax = qmax;
    trace.tr = Buf(be, cgst::trace_doubles(b, qmax));
    std::vector<int64_t> its((size_t)b, 0);
    int64_t* it = iters ? iters : its.data();                              // (filled before a breakdown is raised)
    solve_resident("traced conjugate gradients", ctx, op->op, diag, pc, B->buf.p, X->buf.p, b, tol, maxiter, info, INFO_TRACE,
                   relres, it, &trace);
    if (quad_out) {
      its.assign(it, it + b);
      double* tr = trace.tr.p;
      for (int64_t j = 0; j < b - nquad; ++j) its[(size_t)j] = 0;          // the data columns: no quadrature, 0
      if (nquad > 0)
        slq_quadrature(ctx->c, cgst::trace_alpha(tr, b, qmax), cgst::trace_beta(tr, b, qmax), its.data(),
                       cgst::trace_rho0(tr, b, qmax), qmax, b, quad_out);
      be->download2d(quad_out + b, b, cgst::trace_rho0(tr, b, qmax), b, b, 1);
      check_async_errors(ctx->c);
    }
  });
}

int gsi_slq_quadrature(gsi_ctx* ctx, const double* alpha, const double* beta, const int64_t* steps, const double* rho0,
                       int64_t qmax, int64_t b, double* out) {
  return guarded([&] {
    REQUIRE(ctx && alpha && beta && steps && rho0 && out, "gsi_slq_quadrature: NULL argument");
    try {
      slq_quadrature_check(qmax, b);
    } catch (const Error& e) {
      throw Error(e.code, std::string("gsi_slq_quadrature: ") + e.what());
    }
    for (int64_t j = 0; j < b; ++j)
      REQUIRE(steps[j] >= 0 && steps[j] <= qmax, "gsi_slq_quadrature: steps must lie in 0 .. qmax");
    Backend* be = ctx->c.be.get();
    const int64_t nb = qmax * b;
    Buf ad(be, (size_t)nb), bd(be, (size_t)nb), rd(be, (size_t)b);
    be->upload2d(ad.p, nb, alpha, nb, nb, 1);
    be->upload2d(bd.p, nb, beta, nb, nb, 1);
    be->upload2d(rd.p, b, rho0, b, b, 1);
    slq_quadrature(ctx->c, ad.p, bd.p, steps, rd.p, qmax, b, out);
    check_async_errors(ctx->c);
  });
}

int gsi_precond_sample(gsi_ctx* ctx, const gsi_precond* pc, const gsi_mat* G1, const gsi_mat* G2, gsi_mat* Zout) {
  return guarded([&] {
    REQUIRE(ctx && pc && G1 && G2 && Zout, "gsi_precond_sample: NULL argument");
    REQUIRE(pc->ctx == ctx, "gsi_precond_sample: pc belongs to another context");
    REQUIRE(G1->ctx == ctx && G2->ctx == ctx && Zout->ctx == ctx, "gsi_precond_sample: G1, G2 or Zout belongs to another context");
    REQUIRE(G2->rows == pc->pc.n && G2->cols >= 1, "gsi_precond_sample: G2 must have the preconditioner's rows");
    REQUIRE(G1->rows == pc->pc.K && G1->cols == G2->cols, "gsi_precond_sample: G1 must be K x the columns of G2");
    REQUIRE(Zout->rows == G2->rows && Zout->cols == G2->cols, "gsi_precond_sample: Zout must have the shape of G2");
    REQUIRE(Zout != G2 && Zout->buf.p != G2->buf.p && Zout != G1 && Zout->buf.p != G1->buf.p,
            "gsi_precond_sample: Zout must not be G1 or G2");
    precond_sample(pc->pc, G1->buf.p, G2->buf.p, G2->cols, Zout->buf.p);
    check_async_errors(ctx->c);
  });
}
int gsi_precond_logdet(const gsi_precond* pc, double* logdet_out) {
  return guarded([&] {
    REQUIRE(pc && logdet_out, "gsi_precond_logdet: NULL argument");
    *logdet_out = pc->pc.logdet;
  });
}

int gsi_mat_axpy(gsi_ctx* ctx, double alpha, const gsi_mat* X, gsi_mat* Y) {
  return guarded([&] {
    REQUIRE(ctx && X && Y, "gsi_mat_axpy: NULL argument");
    REQUIRE(X->ctx == ctx && Y->ctx == ctx, "gsi_mat_axpy: X or Y belongs to another context");
    REQUIRE(X->rows == Y->rows && X->cols == Y->cols, "gsi_mat_axpy: X and Y must have the same shape");
    ctx->c.be->axpy(X->rows * X->cols, alpha, X->buf.p, Y->buf.p);
  });
}

// ---- diagonal-pivoted Cholesky of a covariance read by entries, and the principal form of a factor ----
int gsi_op_pivoted_cholesky(gsi_ctx* ctx, const gsi_op* op, int64_t K, double tol, gsi_mat* L, int64_t* piv_out, int64_t* info,
                            double* err_out) {
  return guarded([&] {
    if (info) for (int i = 0; i < 6; ++i) info[i] = 0;
    if (err_out) err_out[0] = err_out[1] = err_out[2] = 0.0;
    REQUIRE(ctx && op && L, "gsi_op_pivoted_cholesky: ctx, op or L is NULL");
    REQUIRE(op->op.ctx == &ctx->c, "gsi_op_pivoted_cholesky: op belongs to another context");
    REQUIRE(L->ctx == ctx, "gsi_op_pivoted_cholesky: L belongs to another context");
    pivoted_cholesky_check(op->op, K, tol, L->rows, L->cols);
    const PcholInfo r = pivoted_cholesky(op->op, K, tol, L->buf.p, piv_out);
    if (info) { info[0] = r.rank; info[1] = r.reason; info[2] = r.path; info[3] = r.form; info[4] = r.polls; info[5] = 0; }
    if (err_out) { err_out[0] = r.trace0; err_out[1] = r.trace; err_out[2] = r.dmax; }
    check_async_errors(ctx->c);
    if (r.reason == 4)
      throw Error(GSI_ERR_NOT_POSDEF, r.rank == 0
                      ? std::string("pivoted Cholesky: the diagonal of op holds a non-finite value (step 0)")
                      : "pivoted Cholesky: a non-finite value was met in step " + std::to_string(r.rank - 1) +
                            " (0-based; in its column, in d or in the trace)");
  });
}

int gsi_mat_principal_factor(gsi_ctx* ctx, const gsi_mat* L, int64_t K, gsi_mat* Z_out, double* s_out) {
  return guarded([&] {
    REQUIRE(ctx && L && Z_out, "gsi_mat_principal_factor: ctx, L or Z_out is NULL");
    REQUIRE(L->ctx == ctx && Z_out->ctx == ctx, "gsi_mat_principal_factor: L or Z_out belongs to another context");
    REQUIRE(!ctx->c.comm, "gsi_mat_principal_factor: ctx has a communicator; the factor lives on one rank");
    REQUIRE(K >= 1 && K <= L->cols, "gsi_mat_principal_factor: K must lie in 1 .. the columns of L");
    REQUIRE(K <= L->rows, "gsi_mat_principal_factor: K exceeds the rows of L");
    REQUIRE(Z_out->rows == L->rows && Z_out->cols >= K, "gsi_mat_principal_factor: Z_out must have the rows of L and at least K columns");
    REQUIRE(Z_out != L && Z_out->buf.p != L->buf.p, "gsi_mat_principal_factor: Z_out must not be L");
    Backend* be = ctx->c.be.get();
    Buf S(be, (size_t)K);
    principal_factor(ctx->c, L->buf.p, L->rows, K, Z_out->buf.p, S.p);
    if (s_out) be->download2d(s_out, K, S.p, K, K, 1);
    check_async_errors(ctx->c);
  });
}

int gsi_pcgamat_create(gsi_ctx* ctx, gsi_pcgamat** mat, const double* etas, int64_t nobs, int64_t K, const double* HX,
                       const double* R, int r_is_diag) {
  return guarded([&] {
    REQUIRE(ctx && mat && etas && HX && R, "NULL argument");
    *mat = nullptr;
    REQUIRE(nobs >= 1 && K >= 1, "bad shape");
    Backend* be = ctx->c.be.get();
    std::unique_ptr<gsi_pcgamat> m(new gsi_pcgamat());
    m->ctx = ctx;
    PcgaLowRank& A = m->A;
    A.ctx = &ctx->c; A.nobs = nobs; A.K = K; A.r_diag = (r_is_diag != 0);
    A.E = Buf(be, (size_t)nobs * K);
    A.HX = Buf(be, (size_t)nobs);
    A.R = Buf(be, A.r_diag ? (size_t)nobs : (size_t)nobs * nobs);
    be->upload2d(A.E.p, nobs, etas, nobs, nobs, K);
    be->upload2d(A.HX.p, nobs, HX, nobs, nobs, 1);
    if (A.r_diag) be->upload2d(A.R.p, nobs, R, nobs, nobs, 1);
    else be->upload2d(A.R.p, nobs, R, nobs, nobs, nobs);
    *mat = m.release();
  });
}
int gsi_pcgamat_destroy(gsi_pcgamat* mat) {
  return guarded([&] { delete mat; });
}
int gsi_pcgamat_mul(gsi_ctx* ctx, const gsi_pcgamat* mat, const double* x, double* y) {
  return guarded([&] {
    REQUIRE(ctx && mat && x && y && mat->ctx == ctx, "bad argument");
    Backend* be = ctx->c.be.get();
    const int64_t n1 = mat->A.nobs + 1;
    Buf xd(be, (size_t)n1), yd(be, (size_t)n1);
    be->upload2d(xd.p, n1, x, n1, n1, 1);
    mat->A.mul(xd.p, yd.p);
    be->download2d(y, n1, yd.p, n1, n1, 1);
    check_async_errors(ctx->c);
  });
}
int gsi_pcgamat_lsqr(gsi_ctx* ctx, const gsi_pcgamat* mat, const double* b, double* x_out, int64_t* iters_out) {
  return guarded([&] {
    REQUIRE(ctx && mat && b && x_out && mat->ctx == ctx, "bad argument");
    Backend* be = ctx->c.be.get();
    const int64_t n1 = mat->A.nobs + 1;
    Buf bd(be, (size_t)n1), xd(be, (size_t)n1);
    be->upload2d(bd.p, n1, b, n1, n1, 1);
    LsqrOperator L;
    L.nrows = L.ncols = n1;
    const PcgaLowRank* A = &mat->A;
    L.mul = [A](const double* xin, double* y) { A->mul(xin, y); };
    L.mul_t = L.mul;                                     // the saddle-point matrix is symmetric
    const int64_t it = lsqr(ctx->c, L, bd.p, xd.p, -1);  // maxiter = max(size(A))   IterativeSolvers default
    be->download2d(x_out, n1, xd.p, n1, n1, 1);
    if (iters_out) *iters_out = it;
    check_async_errors(ctx->c);
  });
}

int gsi_pcgamat_solve(gsi_ctx* ctx, const gsi_pcgamat* mat, const double* b, double* x_out, int64_t* info_out) {
  return with_info(info_out, [&](PathInfo& info) {
    REQUIRE(ctx && mat && b && x_out, "gsi_pcgamat_solve: NULL argument");
    REQUIRE(mat->ctx == ctx, "gsi_pcgamat_solve: the matrix belongs to another context");
    if (mat->A.nobs > 32768)
      throw Error(GSI_ERR_ARG, "gsi_pcgamat_solve: nobs = " + std::to_string(mat->A.nobs) +
                                   " is beyond the 32768 the direct solver takes (its workspace is (nobs + 2) x nobs doubles)");
    mat->A.solve(b, x_out, info);
    check_async_errors(ctx->c);
  });
}

int gsi_chol_lower(gsi_ctx* ctx, const double* A, int64_t n, int64_t lda, double* L_out, int64_t* info_out) {
  return with_info(info_out, [&](PathInfo& info) {
    REQUIRE(ctx && A && L_out, "gsi_chol_lower: NULL argument");
    REQUIRE(n >= 1 && lda >= n, "gsi_chol_lower: need n >= 1 and lda >= n");
    REQUIRE(n <= 32768, "gsi_chol_lower: n is beyond 32768");
    chol_lower_host_matrix(ctx->c, A, n, lda, L_out, info);
    check_async_errors(ctx->c);
    throw_chol_outcome(info, info.column, false, nullptr);
  });
}

// ---- xi-basis objects ------------------------------------------------------------------
int gsi_basis_create(gsi_ctx* ctx, gsi_basis** basis, const gsi_mat* Z, int64_t K, int precision) {
  return guarded([&] {
    REQUIRE(ctx && basis && Z && Z->ctx == ctx, "bad argument");
    *basis = nullptr;
    REQUIRE(K >= 1 && K <= Z->cols, "K out of range for this matrix");
    REQUIRE(precision == 64 || precision == 32, "precision must be 64 or 32");
    std::unique_ptr<gsi_basis> b(new gsi_basis());
    b->ctx = ctx; b->n = Z->rows; b->K = K; b->precision = precision; b->Z64 = Z->buf.p;
    if (precision == 32) {
      const size_t count = (size_t)b->n * (size_t)K;
      b->buf32 = Buf(ctx->c.be.get(), (count + 1) / 2);               // fp32 elements in a double-typed allocation
      ctx->c.be->f64_to_f32(Z->buf.p, b->buf32.p, count);
      b->Z64 = nullptr;
    } else {
      b->owner = const_cast<gsi_mat*>(Z);      // shared ownership: gsi_mat_destroy before gsi_basis_destroy is safe
      b->owner->refs += 1;
    }
    *basis = b.release();
  });
}
int gsi_basis_destroy(gsi_basis* basis) {
  return guarded([&] {
    if (!basis) return;
    gsi_mat* owner = basis->owner;
    delete basis;
    mat_unref(owner);
  });
}
int gsi_pcga_params_basis(gsi_ctx* ctx, const gsi_basis* basis, const double* s, const double* X, double delta,
                          double* out) {
  return guarded([&] {
    REQUIRE(ctx && basis && s && X && out && basis->ctx == ctx, "bad argument");
    basis_params(ctx->c, basis->ref(), s, X, delta, out);
  });
}
int gsi_pcga_update_basis(gsi_ctx* ctx, const gsi_basis* basis, const double* X, double beta_bar, const double* etas,
                          int64_t nobs, const double* xi_bar, double* s_out) {
  return guarded([&] {
    REQUIRE(ctx && basis && X && etas && xi_bar && s_out && basis->ctx == ctx && nobs >= 1, "bad argument");
    basis_update(ctx->c, basis->ref(), X, beta_bar, etas, nobs, xi_bar, s_out);
  });
}
int gsi_basis_download_col(gsi_ctx* ctx, const gsi_basis* basis, int64_t col, double* host) {
  return guarded([&] {
    REQUIRE(ctx && basis && host && basis->ctx == ctx, "bad argument");
    REQUIRE(col >= 0 && col < basis->K, "column out of range");
    Backend* be = ctx->c.be.get();
    const int64_t n = basis->n;
    if (basis->precision == 64) {
      be->download2d(host, n, basis->Z64 + (size_t)col * n, n, n, 1);
      return;
    }
    // unit weight on column `col`: the fp32 column widened exactly
    std::vector<double> w((size_t)basis->K, 0.0), zero((size_t)n, 0.0);
    w[(size_t)col] = 1.0;
    Buf wd(be, (size_t)basis->K), Xd(be, (size_t)n), sd(be, (size_t)n);
    be->upload2d(wd.p, basis->K, w.data(), basis->K, basis->K, 1);
    be->fill_zero(Xd.p, (size_t)n);
    be->basis_gemv_f32(basis->buf32.p, n, basis->K, wd.p, 0.0, Xd.p, sd.p);
    be->download2d(host, n, sd.p, n, n, 1);
  });
}

// ---- sparse forward models ------------------------------------------------------
int gsi_fwd_linear_create(gsi_ctx* ctx, gsi_fwd** fwd, int64_t nobs, int64_t n, const int64_t* rowptr, const int64_t* colidx,
                          const double* vals, const double* weights, int link) {
  return guarded([&] {
    REQUIRE(ctx && fwd, "gsi_fwd_linear_create: ctx / fwd is NULL");
    *fwd = nullptr;
    std::unique_ptr<gsi_fwd> f(new gsi_fwd());
    f->ctx = ctx;
    fwd_create(ctx->c, f->m, nobs, n, rowptr, colidx, vals, weights, link);
    *fwd = f.release();
  });
}
int gsi_fwd_destroy(gsi_fwd* fwd) {
  return guarded([&] { delete fwd; });
}
int gsi_fwd_info(const gsi_fwd* fwd, int64_t* out, int64_t n_out) {
  return guarded([&] {
    REQUIRE(fwd && out && n_out >= 0, "bad argument");
    const FwdModel& m = fwd->m;
    const int64_t v[8] = {m.nobs, m.n, m.nnz, m.plan.nseg(), m.plan.nsplit, m.last_form, m.host_products, m.products};
    for (int64_t i = 0; i < n_out; ++i) out[i] = i < 8 ? v[i] : 0;
  });
}
int gsi_fwd_apply(gsi_ctx* ctx, const gsi_fwd* fwd, const double* P, int64_t ldp, int64_t ncols, double* out, int64_t ldo) {
  return guarded([&] {
    REQUIRE(ctx && fwd && P && out, "NULL argument");
    REQUIRE(fwd->ctx == ctx, "gsi_fwd_apply: the forward model belongs to another context");
    REQUIRE(ncols >= 1 && ldp >= fwd->m.n && ldo >= fwd->m.nobs, "gsi_fwd_apply: bad ncols / leading dimension");
    fwd_apply(ctx->c, fwd->m, P, ldp, ncols, out, ldo);
    check_async_errors(ctx->c);
  });
}
int gsi_fwd_apply_dev(gsi_ctx* ctx, const gsi_fwd* fwd, const gsi_mat* P, gsi_mat* out) {
  return guarded([&] {
    REQUIRE(ctx && fwd && P && out, "gsi_fwd_apply_dev: NULL argument");
    REQUIRE(fwd->ctx == ctx, "gsi_fwd_apply_dev: the forward model belongs to another context");
    REQUIRE(P->ctx == ctx && out->ctx == ctx, "gsi_fwd_apply_dev: P or out belongs to another context");
    REQUIRE(P != out, "gsi_fwd_apply_dev: P and out must be different matrices");
    const FwdModel& m = fwd->m;
    if (P->rows != m.n || P->cols < 1)
      throw Error(GSI_ERR_ARG, "gsi_fwd_apply_dev: P is " + std::to_string(P->rows) + " x " + std::to_string(P->cols) +
                                   ", the model needs n = " + std::to_string(m.n) + " rows and at least one column");
    if (out->rows != m.nobs || out->cols != P->cols)
      throw Error(GSI_ERR_ARG, "gsi_fwd_apply_dev: out is " + std::to_string(out->rows) + " x " + std::to_string(out->cols) +
                                   ", not nobs x columns of P = " + std::to_string(m.nobs) + " x " + std::to_string(P->cols));
    fwd_apply_dev(ctx->c, m, P->buf.p, P->rows, P->cols, out->buf.p, out->rows);
    check_async_errors(ctx->c);
  });
}
int gsi_fwd_adjoint_dev(gsi_ctx* ctx, const gsi_fwd* fwd, const gsi_mat* V, gsi_mat* G) {
  return guarded([&] {
    REQUIRE(ctx && fwd && V && G, "gsi_fwd_adjoint_dev: NULL argument");
    REQUIRE(fwd->ctx == ctx, "gsi_fwd_adjoint_dev: the forward model belongs to another context");
    REQUIRE(V->ctx == ctx && G->ctx == ctx, "gsi_fwd_adjoint_dev: V or G belongs to another context");
    REQUIRE(V != G, "gsi_fwd_adjoint_dev: V and G must be different matrices");
    const FwdModel& m = fwd->m;
    if (m.link != 0)
      throw Error(GSI_ERR_ARG, "gsi_fwd_adjoint_dev: the model has link = " + std::to_string(m.link) +
                                   " (exp): only a linear model (link = 0) has an adjoint");
    if (V->rows != m.nobs || V->cols < 1)
      throw Error(GSI_ERR_ARG, "gsi_fwd_adjoint_dev: V is " + std::to_string(V->rows) + " x " + std::to_string(V->cols) +
                                   ", the model needs nobs = " + std::to_string(m.nobs) + " rows and at least one column");
    if (G->rows != m.n || G->cols != V->cols)
      throw Error(GSI_ERR_ARG, "gsi_fwd_adjoint_dev: G is " + std::to_string(G->rows) + " x " + std::to_string(G->cols) +
                                   ", not n x columns of V = " + std::to_string(m.n) + " x " + std::to_string(V->cols));
    fwd_adjoint(ctx->c, m, V->buf.p, V->rows, V->cols, G->buf.p, G->rows);
    check_async_errors(ctx->c);
  });
}
int gsi_fwd_adjoint_info(const gsi_fwd* fwd, int64_t* out, int64_t n_out) {
  return guarded([&] {
    REQUIRE(fwd && out && n_out >= 0, "gsi_fwd_adjoint_info: bad argument");
    const FwdModel& m = fwd->m;
    const FwdAdjointPlan& ap = m.aplan;
    const int64_t v[7] = {m.aplan_built ? 1 : 0, m.adj_bytes, ap.nlong(), ap.nchunk(), ap.maxlen, m.adj_products,
                          m.adj_host_products};
    for (int64_t i = 0; i < n_out; ++i) out[i] = i < 7 ? v[i] : 0;
  });
}
// A = H C H' (OP_FWD_COV): C = grid_op's covariance, whose plan is shared, H = the model's matrix, which is
// shared too.  Nothing is allocated here: the model's arrays are resident already, its inverted index comes with the
// first product.
int gsi_op_fwd_cov(gsi_ctx* ctx, gsi_op** op, const gsi_op* grid_op, const gsi_fwd* fwd) {
  return guarded([&] {
    REQUIRE(ctx && op && grid_op && fwd, "gsi_op_fwd_cov: NULL argument");
    *op = nullptr;
    const Operator& C = grid_op->op;
    REQUIRE(C.ctx == &ctx->c, "gsi_op_fwd_cov: the grid operator (grid_op) belongs to another context");
    REQUIRE(fwd->ctx == ctx, "gsi_op_fwd_cov: the forward model (fwd) belongs to another context");
    REQUIRE(C.kind == OP_FFT_COV && C.plan != nullptr,
            "gsi_op_fwd_cov: grid_op must be an FFT covariance operator (gsi_op_fft_powerlaw[_fftrf], gsi_op_fft_gridcov[_table])");
    REQUIRE(!ctx->c.comm, "gsi_op_fwd_cov: one GPU only -- not available on a context with a communicator");
    REQUIRE(C.fft_ndims == 2 || C.fft_ndims == 3, "gsi_op_fwd_cov: grid_op must have 2 or 3 axes (a 1-D grid is not supported)");
    const FwdModel& m = fwd->m;
    if (m.n != C.n)
      throw Error(GSI_ERR_ARG, "gsi_op_fwd_cov: fwd has n = " + std::to_string(m.n) + " cells, the grid of grid_op n_grid = " +
                                   std::to_string(C.n));
    if (m.link != 0)
      throw Error(GSI_ERR_ARG, "gsi_op_fwd_cov: fwd has link = " + std::to_string(m.link) +
                                   " (exp): H C H' needs a linear model (link = 0)");
    std::unique_ptr<gsi_op> o(new gsi_op());
    Operator& A = o->op;
    A.ctx = &ctx->c; A.kind = OP_FWD_COV; A.m = m.nobs; A.n = m.nobs; A.row0 = 0; A.mloc = m.nobs; A.ld = 0;
    A.fft_ndims = C.fft_ndims;
    for (int a = 0; a < 3; ++a) A.fft_N[a] = C.fft_N[a];
    A.plan = C.plan;
    A.plan_ref = C.plan_ref;
    A.fwd = fwd->shared;
    *op = o.release();
  });
}
int gsi_pcga_forward_basis(gsi_ctx* ctx, const gsi_basis* basis, const gsi_fwd* fwd, const double* s, const double* X,
                           double delta, double* results_out) {
  return guarded([&] {
    REQUIRE(ctx && basis && fwd && s && X && results_out, "NULL argument");
    REQUIRE(basis->ctx == ctx, "gsi_pcga_forward_basis: the basis belongs to another context");
    REQUIRE(fwd->ctx == ctx, "gsi_pcga_forward_basis: the forward model belongs to another context");
    if (fwd->m.n != basis->n)
      throw Error(GSI_ERR_ARG, "gsi_pcga_forward_basis: the forward model has n = " + std::to_string(fwd->m.n) +
                                   ", the basis n = " + std::to_string(basis->n));
    fwd_forward_basis(ctx->c, fwd->m, basis->ref(), s, X, delta, results_out);
    check_async_errors(ctx->c);
  });
}

// ---- the posterior variance from the resident basis ------------------------------
int gsi_basis_quadform(gsi_ctx* ctx, const gsi_basis* basis, const double* W, int64_t ldw, int64_t ncols, int upper,
                       const double* u, double* a_out, double* q_out, double* t_out, int64_t* info_out) {
  return with_info(info_out, [&](PathInfo& info) {
    REQUIRE(ctx && basis && W && a_out, "gsi_basis_quadform: NULL argument");
    REQUIRE((u == nullptr) == (t_out == nullptr), "gsi_basis_quadform: u and t_out go together");
    REQUIRE(basis->ctx == ctx, "gsi_basis_quadform: the basis belongs to another context");
    REQUIRE(ncols >= 1 && ldw >= basis->K, "gsi_basis_quadform: need ncols >= 1 and ldw >= K");
    basis_quadform(ctx->c, basis->ref(), W, ldw, ncols, upper != 0, u, a_out, q_out, t_out, info);
    check_async_errors(ctx->c);
  });
}

namespace {
void require_posterior_shape(const gsi_pcgamat* mat, const char* who) {
  if (!mat->A.r_diag && mat->A.nobs > 32768)
    throw Error(GSI_ERR_ARG, std::string(who) + ": nobs = " + std::to_string(mat->A.nobs) +
                                 " with a dense R is beyond the 32768 the Cholesky factorization takes");
}
}  // namespace

int gsi_pcgamat_posterior(gsi_ctx* ctx, const gsi_pcgamat* mat, double* W_out, double* u_out, double* gamma_out,
                          int64_t* info_out) {
  return with_info(info_out, [&](PathInfo& info) {
    REQUIRE(ctx && mat && W_out && u_out && gamma_out, "gsi_pcgamat_posterior: NULL argument");
    REQUIRE(mat->ctx == ctx, "gsi_pcgamat_posterior: the matrix belongs to another context");
    require_posterior_shape(mat, "gsi_pcgamat_posterior");
    posterior_factor(mat->A, W_out, u_out, gamma_out, info);
    check_async_errors(ctx->c);
  });
}

int gsi_pcga_posterior_variance(gsi_ctx* ctx, const gsi_basis* basis, const gsi_pcgamat* mat, const double* X,
                                const double* prior, double* var_out, int64_t* info_out) {
  return with_info(info_out, [&](PathInfo& info) {
    REQUIRE(ctx && basis && mat && X && var_out, "gsi_pcga_posterior_variance: NULL argument");
    REQUIRE(basis->ctx == ctx, "gsi_pcga_posterior_variance: the basis belongs to another context");
    REQUIRE(mat->ctx == ctx, "gsi_pcga_posterior_variance: the matrix belongs to another context");
    if (mat->A.K != basis->K)
      throw Error(GSI_ERR_ARG, "gsi_pcga_posterior_variance: the matrix has K = " + std::to_string(mat->A.K) +
                                   ", the basis K = " + std::to_string(basis->K));
    require_posterior_shape(mat, "gsi_pcga_posterior_variance");
    posterior_variance(ctx->c, basis->ref(), mat->A, X, prior, var_out, info);
    check_async_errors(ctx->c);
  });
}

// ---- the exact posterior variance of linear inversion and kriging ----------------
int gsi_mat_rowdot_acc(gsi_ctx* ctx, const gsi_mat* A, const gsi_mat* B, gsi_mat* acc) {
  return guarded([&] {
    REQUIRE(ctx && A && B && acc, "gsi_mat_rowdot_acc: NULL argument");
    REQUIRE(A->ctx == ctx && B->ctx == ctx && acc->ctx == ctx, "gsi_mat_rowdot_acc: A, B or acc belongs to another context");
    if (B->rows != A->rows || B->cols != A->cols)
      throw Error(GSI_ERR_ARG, "gsi_mat_rowdot_acc: B is " + std::to_string(B->rows) + " x " + std::to_string(B->cols) +
                                   ", A is " + std::to_string(A->rows) + " x " + std::to_string(A->cols) +
                                   ": the panels must have the same shape");
    if (acc->rows != A->rows || acc->cols != 1)
      throw Error(GSI_ERR_ARG, "gsi_mat_rowdot_acc: acc is " + std::to_string(acc->rows) + " x " + std::to_string(acc->cols) +
                                   ", not rows of A x 1 = " + std::to_string(A->rows) + " x 1");
    REQUIRE(acc != A && acc != B && acc->buf.p != A->buf.p && acc->buf.p != B->buf.p, "gsi_mat_rowdot_acc: acc must not be A or B");
    rowdot_acc(ctx->c, A->rows, A->cols, A->buf.p, A->rows, B->buf.p, B->rows, acc->buf.p);
    check_async_errors(ctx->c);
  });
}

// ---- the bilinear forms of the likelihood gradient ----------------------------------
static void require_bilinear_g(const char* who, int64_t g, int64_t b) {
  if (g < 0 || g > b || g > 16)
    throw Error(GSI_ERR_ARG, std::string(who) + ": g = " + std::to_string(g) + " must be in 0 .. min(b, 16), b = " + std::to_string(b));
}
static void require_finite_diag(const char* who, const double* dd, int64_t n) {
  if (dd)
    for (int64_t i = 0; i < n; ++i)
      if (!std::isfinite(dd[i])) throw Error(GSI_ERR_ARG, std::string(who) + ": the diagonal holds a non-finite value");
}

int gsi_mat_copy_cols(gsi_ctx* ctx, gsi_mat* dst, int64_t dst_col0, const gsi_mat* src, int64_t src_col0, int64_t ncols) {
  return guarded([&] {
    REQUIRE(ctx && dst && src, "gsi_mat_copy_cols: NULL argument");
    REQUIRE(dst->ctx == ctx && src->ctx == ctx, "gsi_mat_copy_cols: dst or src belongs to another context");
    REQUIRE(dst != src && dst->buf.p != src->buf.p, "gsi_mat_copy_cols: dst must not be src");
    REQUIRE(dst->rows == src->rows, "gsi_mat_copy_cols: dst and src must have the same number of rows");
    REQUIRE(ncols >= 0 && dst_col0 >= 0 && src_col0 >= 0 && dst_col0 + ncols <= dst->cols && src_col0 + ncols <= src->cols,
            "gsi_mat_copy_cols: the column ranges must lie inside dst and src");
    if (ncols == 0 || dst->rows == 0) return;
    const int64_t n = dst->rows;
    ctx->c.be->copy2d(dst->buf.p + (size_t)n * (size_t)dst_col0, n, src->buf.p + (size_t)n * (size_t)src_col0, n, n, ncols);
  });
}

int gsi_mat_bilinear(gsi_ctx* ctx, const gsi_mat* L, const gsi_mat* Y, const gsi_mat* R, const double* dd, int64_t g,
                     double* gram_out, double* t_out) {
  return guarded([&] {
    REQUIRE(ctx && L && Y, "gsi_mat_bilinear: ctx, L or Y is NULL");
    REQUIRE(L->ctx == ctx && Y->ctx == ctx && (R == nullptr || R->ctx == ctx), "gsi_mat_bilinear: L, Y or R belongs to another context");
    REQUIRE(L->rows >= 1 && L->cols >= 1, "gsi_mat_bilinear: L must have at least one row and one column");
    REQUIRE(Y->rows == L->rows && Y->cols == L->cols, "gsi_mat_bilinear: Y must have the shape of L");
    REQUIRE(R == nullptr || (R->rows == L->rows && R->cols == L->cols), "gsi_mat_bilinear: R must have the shape of L");
    REQUIRE(dd == nullptr || R != nullptr, "gsi_mat_bilinear: dd needs R");
    require_bilinear_g("gsi_mat_bilinear", g, L->cols);
    REQUIRE(g == 0 || gram_out != nullptr, "gsi_mat_bilinear: gram_out is NULL with g > 0");
    REQUIRE(g == L->cols || t_out != nullptr, "gsi_mat_bilinear: t_out is NULL with g < b");
    require_finite_diag("gsi_mat_bilinear", dd, L->rows);
    bilinear_terms(ctx->c, L->rows, L->cols, g, L->buf.p, Y->buf.p, R ? R->buf.p : nullptr, dd, gram_out, t_out);
    check_async_errors(ctx->c);
  });
}

int gsi_op_bilinear_terms(gsi_ctx* ctx, const gsi_op* dop, const double* ddiag, const gsi_mat* X, int64_t g, const gsi_mat* Wz,
                          double* gram_out, double* t_out) {
  return guarded([&] {
    REQUIRE(ctx && X, "gsi_op_bilinear_terms: ctx or X is NULL");
    REQUIRE(!ctx->c.comm, "gsi_op_bilinear_terms: one GPU only -- ctx has a communicator");
    REQUIRE(X->ctx == ctx && (Wz == nullptr || Wz->ctx == ctx), "gsi_op_bilinear_terms: X or Wz belongs to another context");
    REQUIRE(dop == nullptr || dop->op.ctx == &ctx->c, "gsi_op_bilinear_terms: dop belongs to another context");
    const int64_t n = X->rows, b = X->cols;
    REQUIRE(n >= 1 && b >= 1, "gsi_op_bilinear_terms: X must have at least one row and one column");
    require_bilinear_g("gsi_op_bilinear_terms", g, b);
    REQUIRE(b == g || Wz != nullptr, "gsi_op_bilinear_terms: Wz is NULL with g < X's columns");
    if (Wz != nullptr && (Wz->rows != n || Wz->cols != b - g))
      throw Error(GSI_ERR_ARG, "gsi_op_bilinear_terms: Wz is " + std::to_string(Wz->rows) + " x " + std::to_string(Wz->cols) +
                                   ", not rows of X x (columns of X - g) = " + std::to_string(n) + " x " + std::to_string(b - g));
    if (dop != nullptr && (dop->op.m != n || dop->op.n != n))
      throw Error(GSI_ERR_ARG, "gsi_op_bilinear_terms: dop is " + std::to_string(dop->op.m) + " x " + std::to_string(dop->op.n) +
                                   ", X has " + std::to_string(n) + " rows");
    REQUIRE(g == 0 || gram_out != nullptr, "gsi_op_bilinear_terms: gram_out is NULL with g > 0");
    REQUIRE(g == b || t_out != nullptr, "gsi_op_bilinear_terms: t_out is NULL with g < X's columns");
    require_finite_diag("gsi_op_bilinear_terms", ddiag, n);
    op_bilinear_terms(ctx->c, dop ? &dop->op : nullptr, ddiag, X->buf.p, n, b, g, Wz ? Wz->buf.p : nullptr, gram_out, t_out);
    check_async_errors(ctx->c);
  });
}

int gsi_op_posterior_variance(gsi_ctx* ctx, const gsi_op* op, const double* diag, const double* X, int64_t ldx, int64_t p,
                              int64_t batch, double* var_out, int64_t* info_out) {
  PostxInfo info;
  if (info_out) for (int i = 0; i < 8; ++i) info_out[i] = 0;
  const int st = guarded([&] {
    REQUIRE(ctx && op && var_out, "gsi_op_posterior_variance: ctx, op or var_out is NULL");
    const Operator& A = op->op;
    REQUIRE(A.ctx == &ctx->c, "gsi_op_posterior_variance: op belongs to another context");
    REQUIRE(A.kind == OP_FWD_COV || A.kind == OP_FFT_COV_AT,
            "gsi_op_posterior_variance: op must be an operator H C H' of gsi_op_fwd_cov or W C W' of gsi_op_fft_at");
    REQUIRE(!ctx->c.comm, "gsi_op_posterior_variance: one GPU only -- ctx has a communicator");
    if (A.n > 32768)
      throw Error(GSI_ERR_ARG, "gsi_op_posterior_variance: op has nobs = " + std::to_string(A.n) +
                                   " rows, beyond the 32768 the Cholesky factorization takes");
    REQUIRE(p >= 0, "gsi_op_posterior_variance: p must be >= 0");
    REQUIRE(p == 0 || X != nullptr, "gsi_op_posterior_variance: X is NULL with p > 0");
    const int64_t n = A.fft_N[0] * A.fft_N[1] * A.fft_N[2];
    if (ldx < n)
      throw Error(GSI_ERR_ARG, "gsi_op_posterior_variance: ldx = " + std::to_string(ldx) + " is smaller than n_grid = " +
                                   std::to_string(n) + ", the rows of X");
    REQUIRE(batch >= 0, "gsi_op_posterior_variance: batch must be >= 0 (0: the operator's own rule)");
    if (diag)
      for (int64_t j = 0; j < A.n; ++j) REQUIRE(std::isfinite(diag[j]), "gsi_op_posterior_variance: diag holds a non-finite value");
    posterior_variance_exact(A, diag, X, ldx, p, batch, var_out, info);
    check_async_errors(ctx->c);
  });
  if (info_out) {
    const int64_t v[6] = {info.column, info.path, info.batches, info.width, info.adjoint_columns, info.trapezoid_bytes};
    for (int i = 0; i < 6; ++i) info_out[i] = v[i];
  }
  return st;
}

// ---- measurement ---------------------------------------------------------------------
int gsi_ctx_profile(gsi_ctx* ctx, int enable) {
  return guarded([&] {
    REQUIRE(ctx, "ctx is NULL");
    ctx->c.be->profile(enable != 0);
    ctx->c.profile_level = enable;
  });
}
int gsi_ctx_phase_reset(gsi_ctx* ctx) {
  return guarded([&] {
    REQUIRE(ctx, "ctx is NULL");
    ctx->c.be->phase_reset();
    if (ctx->c.comm) ctx->c.comm->ncollectives = 0;
    for (int f = 0; f < (int)Context::LU_FORMS; ++f) ctx->c.lu_form_count[f] = 0;
  });
}
int gsi_ctx_phase_times(gsi_ctx* ctx, double* ms_out, int64_t* count_out) {
  return guarded([&] {
    REQUIRE(ctx && ms_out && count_out, "NULL argument");
    static_assert((int)PH_COUNT == GSI_NUM_PHASES, "phase tables out of sync");
    ctx->c.be->phase_times(ms_out, count_out);
  });
}
int gsi_ctx_counters(gsi_ctx* ctx, int64_t* out4) {
  return guarded([&] {
    REQUIRE(ctx && out4, "NULL argument");
    ctx->c.be->counters(out4);
  });
}
int gsi_ctx_release_cache(gsi_ctx* ctx) {
  return guarded([&] {
    REQUIRE(ctx, "ctx is NULL");
    ctx->c.be->release_cache();
  });
}
int gsi_ctx_device_bytes(gsi_ctx* ctx, int64_t* bytes) {
  return guarded([&] {
    REQUIRE(ctx && bytes, "NULL argument");
    *bytes = ctx->c.be->bytes_in_use();
  });
}

}  // extern "C"
