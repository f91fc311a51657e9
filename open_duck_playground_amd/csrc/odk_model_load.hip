// odk_model_load.hip -- the model side of include/odk.h: ODKM blob -> odk_model (DevModel, shape, height field), the odk_model_* getters and
// the thread's error string.  Host code only: no kernel, no HIP call (the kernels: odk_env_kernels.h, the batch API: odk_engine.hip), so it builds without the
// engine's code-generation switches and, for the CPU, into tools/loader_check.cpp with the sanitizers on.
//
// The blob is the library's one caller-supplied byte stream (layout: model.py): Blob checks every record's bounds once, before anything
// is read through it.  odk_model_load is then a list of stages in blob order; each returns 0 or its refusal, and the order of the
// refusals is part of the interface (tests assert which one a model gets).
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <memory>
#include <string>
#include <vector>

#include "odk_host.h"
#include "odk_obs_layout.h"
#include "odk_shapes.h"

using namespace odk;

// ---- the thread's last error (odk_last_error)
static thread_local std::string g_err;
int odk::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
int odk_fail_(int code, const char* msg) { return fail(code, "%s", msg); }
extern "C" const char* odk_last_error(void) { return g_err.c_str(); }

void odk::obs_sizes_nu(int nu, int env_kind, int* nobs, int* npriv) {
  if (nobs) *nobs = obs_nobs(nu, env_kind == ODK_ENV_STANDING);
  if (npriv) *npriv = obs_npriv(nu, env_kind == ODK_ENV_STANDING);
}

// ---- blob parsing
struct RecHdr { char name[32]; uint32_t dtype, ndim, shape[4]; uint64_t nbytes; };   // dtype: 0 = f64, 1 = i32
static_assert(sizeof(RecHdr) == 64, "the ODKM record header");
struct Blob {
  struct Rec { RecHdr h; const unsigned char* p; };
  std::vector<Rec> recs;                  // every record, bounds checked by open()
  bool ok = true; std::string missing;    // a required record that was absent, of another type or too large: the last one, by name

  // The record table of `len` bytes at `b` (magic checked by the caller).  null, or what is wrong with the first record that does not lie
  // inside the blob -- header, payload and its padding to 8 bytes -- or contradicts itself; nothing is read through such a blob.
  const char* open(const unsigned char* b, uint64_t len) {
    uint32_t n;
    memcpy(&n, b + 8, 4);
    uint64_t off = 16;
    for (uint32_t i = 0; i < n; i++) {
      Rec r;
      if (len - off < 64) return "a record header runs past the end of the blob";
      memcpy(&r.h, b + off, 64);
      off += 64;
      const uint64_t nb = r.h.nbytes, pad = (8 - (nb & 7)) & 7;
      if (nb > len - off || pad > len - off - nb) return "a record's data runs past the end of the blob";   // (no sum that a huge nbytes could wrap)
      if (r.h.ndim > 4) return "a record with more than four dimensions";
      const uint64_t item = r.h.dtype == 0 ? 8 : 4;
      if (r.h.ndim == 2 && r.h.dtype <= 1 && (nb % item != 0 || (uint64_t)r.h.shape[0] * r.h.shape[1] != nb / item)) return "a 2-D record whose shape disagrees with its size";
      r.p = b + off;
      recs.push_back(r);
      off += nb + pad;
    }
    return nullptr;
  }
  const Rec* find(const char* name) const {   // the first record of that name, or null
    for (const Rec& q : recs) if (strncmp(q.h.name, name, 32) == 0) return &q;
    return nullptr;
  }
  // the record of that name if it has that type and holds at most maxc items (its count in *cnt), or null.  A required one that fails is noted in
  // ok / missing; an optional one leaves them alone -- the caller keeps its default.
  const Rec* get(const char* name, uint32_t dtype, int maxc, bool optional, int* cnt) {
    const Rec* r = find(name);
    const bool found = r && r->h.dtype == dtype;
    const uint64_t n = found ? r->h.nbytes / (dtype == 0 ? 8 : 4) : 0;
    if (found && n <= (uint64_t)maxc) { *cnt = (int)n; return r; }
    if (!optional) { ok = false; missing = found ? std::string(name) + " (too large)" : name; }
    return nullptr;
  }
  // typed copies: the item count, -1 without the record
  int F(const char* name, float* dst, int maxc) {
    int cnt; const Rec* r = get(name, 0, maxc, false, &cnt);
    if (!r) return -1;
    for (int i = 0; i < cnt; i++) { double v; memcpy(&v, r->p + 8 * i, 8); dst[i] = (float)v; }
    return cnt;
  }
  int D(const char* name, double* dst, int maxc, bool optional = false) {
    int cnt; const Rec* r = get(name, 0, maxc, optional, &cnt);
    if (!r) return -1;
    memcpy(dst, r->p, 8 * (size_t)cnt);
    return cnt;
  }
  int I(const char* name, int* dst, int maxc, bool optional = false) {
    int cnt; const Rec* r = get(name, 1, maxc, optional, &cnt);
    if (!r) return -1;
    memcpy(dst, r->p, 4 * (size_t)cnt);
    return cnt;
  }
  // scalars (0 without the record) and optional records (dst keeps the caller's default without one)
  int I1(const char* name) { int v = 0; I(name, &v, 1); return v; }
  double D1(const char* name) { double v = 0; D(name, &v, 1); return v; }
  int optI(const char* name, int* dst, int maxc) { return I(name, dst, maxc, true); }
  int optD(const char* name, double* dst, int maxc) { return D(name, dst, maxc, true); }
  // 2D int table [rows][srccols] -> dst[rows][dstcols]
  void I2(const char* name, int* dst, int rows_max, int dstcols) {
    int cnt; const Rec* r = get(name, 1, INT32_MAX, false, &cnt);
    if (!r) return;
    if (r->h.ndim != 2) { ok = false; missing = name; return; }
    int rows = (int)r->h.shape[0], cols = (int)r->h.shape[1];
    if (rows > rows_max || cols > dstcols) { ok = false; missing = std::string(name) + " (shape)"; return; }
    for (int i = 0; i < rows; i++)
      for (int c2 = 0; c2 < cols; c2++) memcpy(&dst[i * dstcols + c2], r->p + 4 * ((size_t)i * cols + c2), 4);
  }
  // optional 2D float table [rows][cols] of any size (the height field): false without one
  bool optF2(const char* name, std::vector<float>& dst, int* rows, int* cols) {
    int cnt; const Rec* r = get(name, 0, INT32_MAX, true, &cnt);
    if (!r || r->h.ndim != 2) return false;
    *rows = (int)r->h.shape[0]; *cols = (int)r->h.shape[1];
    dst.resize((size_t)cnt);
    for (int i = 0; i < cnt; i++) { double v; memcpy(&v, r->p + 8 * (size_t)i, 8); dst[i] = (float)v; }
    return true;
  }
};

static void quat2mat(const double* q, double* m) {
  double w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}
static void make_frame_h(const double* n, float* frame) {
  double a[3] = {n[0], n[1], n[2]}, b[3] = {0, 0, 0}, c[3];
  double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  for (int k = 0; k < 3; k++) a[k] /= na;
  if (fabs(a[1]) < 0.5) b[1] = 1; else b[2] = 1;
  double dt = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  for (int k = 0; k < 3; k++) b[k] -= a[k] * dt;
  double nb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
  for (int k = 0; k < 3; k++) b[k] /= nb;
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
  for (int k = 0; k < 3; k++) { frame[k] = (float)a[k]; frame[3 + k] = (float)b[k]; frame[6 + k] = (float)c[k]; }
}
// constant impedance of a row at pos = 0 (friction loss): returns R, b
static void row_consts(const double* solref, const double* solimp, double dt, double invweight, double* R, double* bb) {
  double timeconst = fmax(solref[0], 2 * dt), dmin = fmin(fmax(solimp[0], 0.0001), 0.9999), dmax = fmin(fmax(solimp[1], 0.0001), 0.9999);
  double b = 2.0 / (dmax * timeconst);
  if (solref[1] <= 0) b = -solref[1] / dmax;
  double imp = dmin;  // imp_x = 0 -> imp_y = 0
  *R = fmax(invweight * (1 - imp) / imp, 1e-15);
  *bb = b;
}

// mju impedance constants of one constraint row (the same float arithmetic the kernels used to repeat per row and substep)
static void pack_imp(const float* solref, const float* solimp, float dt, float* P) {
  const float timeconst = fmaxf(solref[0], 2.0f * dt), dampratio = solref[1];
  const float dmin = fminf(fmaxf(solimp[0], 0.0001f), 0.9999f), dmax = fminf(fmaxf(solimp[1], 0.0001f), 0.9999f);
  const float width = fmaxf(solimp[2], 1e-15f), mid = fminf(fmaxf(solimp[3], 0.0001f), 0.9999f), power = fmaxf(solimp[4], 1.0f);
  float k = 1.0f / (dmax * dmax * timeconst * timeconst * dampratio * dampratio);
  float b = 2.0f / (dmax * timeconst);
  if (solref[0] <= 0) k = -solref[0] / (dmax * dmax);
  if (solref[1] <= 0) b = -solref[1] / dmax;
  P[0] = k; P[1] = b; P[2] = dmin; P[3] = dmax; P[4] = 1.0f / width; P[5] = mid; P[6] = power;
  P[7] = 1.0f / powf(mid, power - 1.0f); P[8] = 1.0f / powf(1.0f - mid, power - 1.0f);
}

// Twin-dof detection and the reduced (twins merged) tree layouts -- see DevModel::paired.  Called after the dof / joint /
// foot tables are in place.  Returns false when the reduced tree is not "floating base + up to four serial chains of <= 6
// dofs" (the form chain_solve is built for).
namespace {
struct SparseLayout { int depth[MAXV], adr[MAXV], ancmask[MAXV], descmask[MAXV], anc_at[MAXV][MAXV], nnz; };
// rows in dof order; row i = entries for i's ancestors by depth (c = depth[i]: the diagonal) -- tables.py _sparse_layout
void sparse_layout(const int* parent, int n, SparseLayout& L) {
  L.nnz = 0;
  for (int i = 0; i < n; i++) {
    L.depth[i] = parent[i] < 0 ? 0 : L.depth[parent[i]] + 1;
    L.adr[i] = L.nnz; L.nnz += L.depth[i] + 1;
    L.ancmask[i] = 0; L.descmask[i] = 0;
  }
  for (int i = 0; i < n; i++) {
    int a = i;
    for (int c = L.depth[i]; c >= 0; c--, a = parent[a]) {
      L.anc_at[i][c] = a;
      if (a != i) { L.ancmask[i] |= 1 << a; L.descmask[a] |= 1 << i; }
    }
  }
}
}  // namespace
// Body-to-lane layout of forward_env's sweeps for G lanes per env: lane_body[lane] = body id, -1 for a lane without a body.
// The chain scans shift by 1, 2 and 4 lanes with DPP row_shr / row_shl, which never cross a 16-lane row, so every serial
// chain (body_is_path, from its body_path_head on) takes consecutive lanes of ONE row, in chain order: upmask / pathmask
// (offsets along the chain) keep their meaning.  Greedy in body order: a chain starts at the first run of free lanes that
// does not cross a row, every other body takes the lowest free lane.  false: no such layout.
static bool build_body_lanes(const DevModel& m, int G, int* lane_body) {
  for (int l = 0; l < 64; l++) lane_body[l] = -1;
  for (int b = 0; b < m.nb; b++) {
    if (m.body_is_path[b] && !m.body_path_head[b]) continue;   // placed with its chain's head
    int len = 1;
    if (m.body_is_path[b])
      while (b + len < m.nb && m.body_is_path[b + len] && !m.body_path_head[b + len]) len++;
    int at = -1;
    for (int s = 0; s + len <= G && at < 0; s++) {
      if ((s >> 4) != ((s + len - 1) >> 4)) continue;
      bool free = true;
      for (int k = 0; k < len; k++) free = free && lane_body[s + k] < 0;
      if (free) at = s;
    }
    if (at < 0) return false;
    for (int k = 0; k < len; k++) lane_body[at + k] = b + k;
  }
  return true;
}
// DevModel::body_st: what forward_env's sweeps need of each body, flattened, in lane order for G = 32 and G = 64 (a lane
// without a body gets a record with level -2 and body -1).  false: a body-to-lane layout does not exist.
static bool fill_body_st(DevModel& m) {
  auto fill = [&](BodySt& b, int bi, bool in) {
    memset(&b, 0, sizeof(b));
    b.level = in ? m.body_level[bi] : -2;
    b.parent = m.body_parent[bi];
    b.pathmask = in ? m.body_pathmask[bi] : 0;
    b.is_path = in ? m.body_is_path[bi] : 0;
    b.upmask = in ? m.body_upmask[bi] : 0;
    b.path_head = in ? m.body_path_head[bi] : 0;
    for (int k = 0; k < 4; k++) b.child[k] = m.body_children[bi][k];
    b.njnt = (in && b.level > 0) ? m.body_jntnum[bi] : 0;
    for (int k = 0; k < 2; k++) {
      const bool on = k < b.njnt;
      const int j = on ? m.body_jntadr[bi] + k : 0;
      b.jj[k] = j;
      b.jd[k] = m.jnt_dofadr[j];
      b.jr[k] = (m.paired && m.dof_tkind[b.jd[k]] == 2) ? -1 : m.dof_red[b.jd[k]];
      for (int c = 0; c < 3; c++) b.ax[k][c] = on ? m.jnt_axis[j][c] : 0.0f;
    }
    for (int c = 0; c < 3; c++) { b.pos[c] = m.body_pos[bi][c]; b.ipos[c] = m.body_ipos[bi][c]; }
    for (int c = 0; c < 4; c++) b.quat[c] = m.body_quat[bi][c];
    for (int c = 0; c < 6; c++) b.inertia[c] = m.body_inertia[bi][c];
  };
  for (int g = 0; g < 2; g++) {
    int lane_body[64];
    if (!build_body_lanes(m, g ? 64 : 32, lane_body)) return false;
    for (int l = 0; l < 64; l++) {
      const int bi = lane_body[l];
      fill(m.body_st[g][l], bi >= 0 ? bi : 0, bi >= 0);
      m.body_st[g][l].body = bi;
    }
  }
  return true;
}

static bool build_reduced_tables(DevModel& m) {
  m.paired = 0; m.nrchain = 0;
  int ntwin = 0;
  for (int d = 0; d < MAXV; d++) { m.dof_tkind[d] = 0; m.dof_red[d] = 0; m.red_main[d] = 0; m.red_twin[d] = -1; }
  for (int v = 7; v < m.nv; v++) {
    const int u = v - 1, ju = m.dof_jnt[u], jv = m.dof_jnt[v];
    if (ju < 0 || jv < 0 || m.dof_tkind[u] != 0) continue;
    const bool same = m.dof_body[u] == m.dof_body[v] && m.dof_anc[v][1] == u && m.jnt_axis[ju][0] == m.jnt_axis[jv][0] &&
                      m.jnt_axis[ju][1] == m.jnt_axis[jv][1] && m.jnt_axis[ju][2] == m.jnt_axis[jv][2];   // jnt_pos == 0 for every hinge (checked by the caller)
    if (!same) continue;
    m.dof_tkind[u] = 1; m.dof_tkind[v] = 2; ntwin++;
  }
  m.paired = ntwin > 0;
  int nr = 0;
  for (int d = 0; d < m.nv; d++) {
    if (m.dof_tkind[d] == 2) { m.dof_red[d] = m.dof_red[d - 1]; continue; }
    m.dof_red[d] = nr; m.red_main[nr] = d; m.red_twin[nr] = m.dof_tkind[d] == 1 ? d + 1 : -1; nr++;
  }
  m.nvr = nr;
  int rparent[MAXV], rvparent[MAXV];
  for (int r = 0; r < nr; r++) {
    const int p = m.dof_anc[m.red_main[r]][1];   // -1 at the root
    rparent[r] = p < 0 ? -1 : m.dof_red[p];
    rvparent[r] = rparent[r];
    const int u = m.red_main[r];
    m.red_foot[r] = m.foot_dofmask[0][u] | (m.foot_dofmask[1][u] << 1);
  }
  // virtual tree (tables.py): the second leg hangs below the first foot's last dof
  {
    int l_last = -1, r_first = -1;
    for (int r = 0; r < nr; r++) {
      if (m.red_foot[r] & 1) l_last = r;
      if ((m.red_foot[r] & 2) && !(m.red_foot[r] & 1) && r_first < 0) r_first = r;
    }
    if (l_last >= 0 && r_first > l_last) rvparent[r_first] = l_last;
  }
  static SparseLayout T, V;   // model loading is not re-entrant anyway (thread-local error string aside)
  sparse_layout(rparent, nr, T);
  sparse_layout(rvparent, nr, V);
  if (T.nnz > MAXNZ || V.nnz > MAXNZ) return false;
  m.nMr = T.nnz; m.nHr = V.nnz;
  for (int r = 0; r < nr; r++) {
    m.red_depth[r] = T.depth[r]; m.red_Madr[r] = T.adr[r]; m.red_ancmask[r] = T.ancmask[r]; m.red_descmask[r] = T.descmask[r];
    m.rv_depth[r] = V.depth[r]; m.rv_Madr[r] = V.adr[r]; m.rv_ancmask[r] = V.ancmask[r]; m.rv_descmask[r] = V.descmask[r];
  }
  auto pack = [&](int r, int a) {
    const bool diag = a == r, pair = diag && m.red_twin[r] >= 0;
    return r | (a << 5) | (m.red_foot[r] << 10) | (m.red_foot[a] << 12) | ((int)diag << 14) | ((int)pair << 15) | (m.red_main[r] << 16);
  };
  for (int r = 0; r < nr; r++) {
    for (int c = 0; c <= T.depth[r]; c++) m.R_ent[T.adr[r] + c] = pack(r, T.anc_at[r][c]);
    for (int c = 0; c <= V.depth[r]; c++) {
      const int a = V.anc_at[r][c];
      int src = -1;   // address of (r, a) in the true reduced layout, if a is a true ancestor (or r itself)
      if (a == r || ((T.ancmask[r] >> a) & 1)) src = T.adr[r] + T.depth[a];
      m.RH_ent[V.adr[r] + c] = pack(r, a) | ((src + 1) << 21);
    }
  }
  // reduced chains below the floating base
  int d = 6;
  bool ok = nr > 6;
  for (int r = 0; r < 6 && ok; r++) ok = rparent[r] == r - 1;
  while (ok && d < nr) {
    if (rparent[d] != 5 || m.nrchain == 4) { ok = false; break; }
    int e = d;
    while (e + 1 < nr && rparent[e + 1] == e) e++;
    m.rchain_first[m.nrchain] = d; m.rchain_len[m.nrchain] = e - d + 1; m.nrchain++;
    if (e - d + 1 > 6) ok = false;      // (the chosen shape's own chain length is checked once the shape is known)
    d = e + 1;
  }
  // the reduced dofs above a foot must be exactly the six base dofs + one whole chain (foot_twist in odk_kernels.h)
  for (int f = 0; f < 2 && ok; f++) {
    int c = -1;
    for (int k = 0; k < m.nrchain; k++) if ((m.red_foot[m.rchain_first[k]] >> f) & 1) c = k;
    ok = c >= 0;
    for (int r = 0; r < nr && ok; r++) {
      const bool want = r < 6 || (r >= m.rchain_first[c] && r < m.rchain_first[c] + m.rchain_len[c]);
      ok = (((m.red_foot[r] >> f) & 1) != 0) == want;
    }
    if (ok) { m.foot_rchain_first[f] = m.rchain_first[c]; m.foot_rchain_len[f] = m.rchain_len[c]; }
  }
  if (ok && !m.paired) {   // a model without twins reduces to itself: the tables above must be the blob's own (tables.py)
    ok = m.nMr == m.nM && m.nHr == m.nH;
    for (int r = 0; r < nr && ok; r++)
      ok = m.red_depth[r] == m.dof_depth[r] && m.red_Madr[r] == m.dof_Madr[r] && m.red_ancmask[r] == m.dof_ancmask[r] && m.red_descmask[r] == m.dof_descmask[r] &&
           m.rv_depth[r] == m.vdof_depth[r] && m.rv_Madr[r] == m.vdof_Madr[r] && m.rv_ancmask[r] == m.vdof_ancmask[r] && m.rv_descmask[r] == m.vdof_descmask[r];
    for (int p = 0; p < m.nM && ok; p++) ok = (m.R_ent[p] & 31) == m.M_i[p] && ((m.R_ent[p] >> 5) & 31) == m.M_j[p];
    for (int p = 0; p < m.nH && ok; p++) ok = (m.RH_ent[p] & 31) == m.H_i[p] && ((m.RH_ent[p] >> 5) & 31) == m.H_j[p] && (m.RH_ent[p] >> 21) - 1 == m.H_src[p];
  }
  return ok;
}

// Face polygons and unique edges of a convex hull given as outward triangles (what mjx mesh.py prepares for collision_convex:
// coplanar facets merged, edges with their two faces).  Triangles that share an edge and a plane (normals within 1e-6) become one
// polygon (at most a quad here: larger merges are refused).  Order matters downstream (first-index tie-breaks): faces in order of
// their first triangle, polygons start at the first boundary edge, edges in face order with va < vb.
static bool build_convex_tables(const double (*v)[3], int nv, const int (*tri)[3], int nt, int* npoly, int (*poly)[5], float (*fnorm)[3], int* nedge,
                                int (*edge)[4], float* centroid, int maxf, int maxe) {
  std::vector<std::array<double, 3>> tn(nt);
  std::vector<int> grp(nt);
  double c[3] = {0, 0, 0};
  for (int i = 0; i < nv; i++) for (int k = 0; k < 3; k++) c[k] += v[i][k] / nv;
  for (int k = 0; k < 3; k++) centroid[k] = (float)c[k];
  for (int t = 0; t < nt; t++) {
    double e1[3], e2[3], n[3];
    for (int k = 0; k < 3; k++) { e1[k] = v[tri[t][1]][k] - v[tri[t][0]][k]; e2[k] = v[tri[t][2]][k] - v[tri[t][0]][k]; }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1]; n[1] = e1[2] * e2[0] - e1[0] * e2[2]; n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double l = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (l == 0) return false;
    tn[t] = {n[0] / l, n[1] / l, n[2] / l};
    grp[t] = t;
  }
  for (int it = 0; it < nt; it++)
    for (int a = 0; a < nt; a++)
      for (int b = a + 1; b < nt; b++) {
        if (grp[a] == grp[b]) continue;
        int shared = 0;
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) if (tri[a][i] == tri[b][j]) shared++;
        if (shared == 2 && fabs(tn[a][0] - tn[b][0]) < 1e-6 && fabs(tn[a][1] - tn[b][1]) < 1e-6 && fabs(tn[a][2] - tn[b][2]) < 1e-6) {
          const int ga = grp[a], gb = grp[b], lo = ga < gb ? ga : gb;
          for (int t = 0; t < nt; t++) if (grp[t] == ga || grp[t] == gb) grp[t] = lo;
        }
      }
  int nf = 0;
  for (int g = 0; g < nt; g++) {
    std::vector<int> ea, eb;
    bool any = false;
    for (int t = 0; t < nt; t++) {
      if (grp[t] != g) continue;
      any = true;
      for (int i = 0; i < 3; i++) {
        const int a = tri[t][i], b = tri[t][(i + 1) % 3];
        bool inner = false;
        for (int u = 0; u < nt && !inner; u++) {
          if (grp[u] != g || u == t) continue;
          for (int j = 0; j < 3; j++) if (tri[u][j] == b && tri[u][(j + 1) % 3] == a) inner = true;
        }
        if (!inner) { ea.push_back(a); eb.push_back(b); }
      }
    }
    if (!any) continue;
    if (nf >= maxf || ea.size() > 4) return false;
    int cur = ea[0], cnt = 0;
    for (size_t step = 0; step < ea.size(); step++) {
      poly[nf][1 + cnt++] = cur;
      int nxt = -1;
      for (size_t k = 0; k < ea.size(); k++) if (ea[k] == cur) { nxt = eb[k]; break; }
      cur = nxt;
      if (cur == ea[0] || cur < 0) break;
    }
    poly[nf][0] = cnt;
    for (int k = cnt; k < 4; k++) poly[nf][1 + k] = poly[nf][1];
    for (int k = 0; k < 3; k++) fnorm[nf][k] = (float)tn[g][k];
    nf++;
  }
  int ne = 0;
  for (int f = 0; f < nf; f++)
    for (int i = 0; i < poly[f][0]; i++) {
      const int a = poly[f][1 + i], b = poly[f][1 + (i + 1) % poly[f][0]];
      if (a > b) continue;
      if (ne >= maxe) return false;
      edge[ne][0] = a; edge[ne][1] = b; edge[ne][2] = f; edge[ne][3] = -1; ne++;
    }
  for (int f = 0; f < nf; f++)
    for (int i = 0; i < poly[f][0]; i++) {
      const int a = poly[f][1 + i], b = poly[f][1 + (i + 1) % poly[f][0]];
      if (a < b) continue;
      bool found = false;
      for (int k = 0; k < ne; k++) if (edge[k][0] == b && edge[k][1] == a) { edge[k][3] = f; found = true; }
      if (!found) return false;   // open surface
    }
  for (int k = 0; k < ne; k++) if (edge[k][2] < 0 || edge[k][3] < 0) return false;
  *npoly = nf; *nedge = ne;
  return true;
}

// DevModel::obs_tab: the observation layouts (joystick.py:570-615 / standing.py:524-565) as gather entries, one per output
// element, for both tasks.  Joystick, nu actuators: gyro 3 (noisy) | accelerometer 3 (noisy) | command 7 | joint angles - default nu (noisy; the
// backlash twin's angle added where the actuator has one) | joint velocities nu (noisy, scaled) | last_act, last_last_act, last_last_last_act,
// motor_targets nu each | contact 2 | phase 2; privileged tail: gyro, accelerometer, gravity, local linvel, global angvel 3 each | joint angles -
// default nu | joint velocities nu | root height 1 | actuator forces nu | contact 2 | feet linvel 6 | air time 2 | reference motion 40 |
// imitation counter 1 | phase 2.  Standing = the same minus motor_targets, the observed phase, reference motion, counter and privileged phase.
template <class S> static void build_obs_table(DevModel& m) {
  using E = EnvL<S>;
  constexpr int NU = S::NU;
  constexpr RecLay RL = rec_lay(NU);
  constexpr int NOBS = obs_nobs(NU, false);
  namespace PA = priv_at;   // the privileged tail's boundaries: odk_obs_layout.h, which the report kernels read the rows by
  static_assert(obs_npriv(NU, false) <= OBS_MAX && draw_count(NU) < 255 && 3 + NU <= 32, "ObsEnt");
  static_assert(obs_npriv(NU, true) == obs_nobs(NU, true) + PA::ref_frame(NU) && obs_npriv(NU, false) == NOBS + PA::imitation_counter(NU) + 3 &&
                obs_at::last_act(NU) + 4 * NU + 4 == NOBS, "odk_obs_layout.h");
  const int MISC = S::O_SCR + S::S_MISC, INFO = E::O_INFO, SENS = S::O_SENS;
  for (int kind = 0; kind < 2; kind++) {
    const bool standing = kind != 0;
    const int NP = obs_npriv(NU, standing);
    for (int ks = 0; ks < OBS_MAX; ks++) {
      ObsEnt e = {0, -1, 0.0f, 0};
      if (ks < NP) {
        const int k = !standing ? ks : (ks < 13 + 5 * NU ? ks : (ks < 15 + 5 * NU ? ks + NU : ks + NOBS - (15 + 5 * NU)));
        const int q = k - NOBS;
        auto noise = [&](int draw, int kind_) { e.fl |= (draw - 4 + 1) | kind_ << 8; };   // (draw i sits at NZ[i - 4])
        auto joint = [&](int u) {
          e.a = S::O_QPOS + m.act_qposadr[u];
          if (m.act_backlash_qposadr[u] >= 0) e.b = S::O_QPOS + m.act_backlash_qposadr[u]; else e.fl |= OBS_FL_PLUS0;
          e.kc = m.key_ctrl[u];
        };
        if (k < 3) { e.a = SENS + m.adr_gyro + k; noise(4 + k, 0); }
        else if (k < 6) { e.a = SENS + m.adr_accelerometer + k - 3; noise(4 + k, 1); }
        else if (k < 13) e.a = INFO + RL.CMD + k - 6;
        else if (k < 13 + NU) { const int u = k - 13; joint(u); noise(13 + u, 3 + u); }
        else if (k < 13 + 2 * NU) { const int u = k - 13 - NU; e.a = S::O_QVEL + m.act_dofadr[u]; noise(draw_qvel(NU) + u, 2); e.fl |= OBS_FL_VEL; }
        else if (k < 13 + 3 * NU) e.a = INFO + RL.LAST + k - 13 - 2 * NU;
        else if (k < 13 + 4 * NU) e.a = INFO + RL.LAST2 + k - 13 - 3 * NU;
        else if (k < 13 + 5 * NU) e.a = INFO + RL.LAST3 + k - 13 - 4 * NU;
        else if (k < 13 + 6 * NU) e.a = INFO + RL.MT + k - 13 - 5 * NU;
        else if (k < 15 + 6 * NU) e.a = MISC + OBS_PARK_CON + k - 13 - 6 * NU;
        else if (k < 17 + 6 * NU) e.a = MISC + OBS_PARK_PHASE + k - 15 - 6 * NU;
        else if (q < PA::ACCELEROMETER) e.a = SENS + m.adr_gyro + q - PA::GYRO;
        else if (q < PA::GRAVITY) e.a = SENS + m.adr_accelerometer + q - PA::ACCELEROMETER;
        else if (q < PA::LOCAL_LINVEL) e.a = MISC + 10 + q - PA::GRAVITY;
        else if (q < PA::GLOBAL_ANGVEL) e.a = SENS + m.adr_local_linvel + q - PA::LOCAL_LINVEL;
        else if (q < PA::JOINT_POS) e.a = SENS + m.adr_global_angvel + q - PA::GLOBAL_ANGVEL;
        else if (q < PA::joint_vel(NU)) joint(q - PA::JOINT_POS);
        else if (q < PA::root_height(NU)) e.a = S::O_QVEL + m.act_dofadr[q - PA::joint_vel(NU)];
        else if (q < PA::actuator_force(NU)) e.a = S::O_QPOS + 2;
        else if (q < PA::contact(NU)) e.a = S::O_ACTF + q - PA::actuator_force(NU);
        else if (q < PA::feet_linvel(NU)) e.a = MISC + OBS_PARK_CON + q - PA::contact(NU);
        else if (q < PA::air_time(NU)) { const int t = q - PA::feet_linvel(NU); e.a = SENS + m.adr_foot_linvel[t >= 3 ? 1 : 0] + (t >= 3 ? t - 3 : t); }
        else if (q < PA::ref_frame(NU)) e.a = INFO + RL.AIR + q - PA::air_time(NU);
        else if (q < PA::imitation_counter(NU)) e.a = E::O_REF + q - PA::ref_frame(NU);
        else if (q == PA::imitation_counter(NU)) e.a = MISC + OBS_PARK_IMI;
        else e.a = MISC + OBS_PARK_PHASE + q - PA::imitation_counter(NU) - 1;
      }
      m.obs_tab[kind][ks] = e;
    }
  }
}

// ---- odk_model_load: the stages, in the order they run.  What one stage reads from the blob and a later one needs travels in Load.
namespace {
struct Load {
  Blob& B; odk_model& mo; DevModel& m;
  double dt = 0; int eulerdamp = 0;                                        // options
  int eq_n = 0, eq_type[16], eq_active[16], eq_o1[16], eq_o2[16];          // <equality>, as compiled
  double eq_data[16 * 11], eq_solref[16 * 2], eq_solimp[16 * 5];
  double dof_iw[MAXV], biw[MAXB * 2];                                      // dof_invweight0, body_invweight0
  int foot_cg[2], floor_cg, cg_type[4], cg_body[4], cg_prio[4];            // collision geoms: the two feet and the floor
  double cg_pos[12], cg_quat[16], cg_fric[12], cg_solref[8], cg_solimp[20], cg_solmix[4];
  bool shape_eq = false;                                                   // the chosen shape carries the optional constraint code (Shape::EQ)
  int body_name[MAXB][32];                                                 // k_body_name: the bodies' names, one character per int (optional; for messages only)
  bool has_names = false;
};
// a body as a refusal names it: 'name' (body 3), or body 3 for a blob without the name table
std::string body_label(const Load& c, int b) {
  std::string s;
  if (c.has_names) {
    s = "'";
    for (int k = 0; k < 32 && c.body_name[b][k] > 0 && c.body_name[b][k] < 128; k++) s += (char)c.body_name[b][k];
    s += "' (";
  }
  s += "body " + std::to_string(b);
  return c.has_names ? s + ")" : s;
}
int missing(const Load& c) { return fail(ODK_ERR_INVALID, "odk_model_load: missing %s", c.B.missing.c_str()); }
const char* const NO_EQ_ROWS = "equality rows are compiled into the third and fourth model shapes only (the duck's kernels carry none)";
// solref / solimp of equality constraint k -> the row's impedance constants
void eq_pack_imp(const Load& c, int k, float* P) {
  float sr[2] = {(float)c.eq_solref[2 * k], (float)c.eq_solref[2 * k + 1]}, si[5];
  for (int a = 0; a < 5; a++) si[a] = (float)c.eq_solimp[5 * k + a];
  pack_imp(sr, si, c.m.dt, P);
}

int load_options(Load& c) {
  Blob& B = c.B; DevModel& m = c.m;
  m.nq = B.I1("nq"); m.nv = B.I1("nv"); m.nu = B.I1("nu"); m.nb = B.I1("nbody"); m.nj = B.I1("njnt"); m.nsite = B.I1("nsite");
  if (!B.ok) return missing(c);
  if (m.nq > MAXQ || m.nv > MAXV || m.nu > MAXU || m.nb > MAXB || m.nj > MAXJ || m.nsite > MAXSITE) return fail(ODK_ERR_UNSUPPORTED, "model too large");
  // <option cone="elliptic">: zones, cone Hessian and exact line search (odk_kernels.h "elliptic cones") are accepted for EVERY compiled shape
  // with hull feet, at 32 lanes per env: the third and fourth shapes carry the code as a runtime switch (Shape::ELL), the duck's two shapes have
  // instantiations of their own with it (ShapeAE / ShapeBE; launch()).  The only refusal is sphere / capsule feet (select_shape, by name).
  int cone = 0;
  B.optI("opt_cone", &cone, 1);
  m.cone = cone != 0;
  c.dt = B.D1("opt_timestep"); m.dt = (float)c.dt;
  double g3[3];
  B.D("opt_gravity", g3, 3); for (int k = 0; k < 3; k++) m.gravity[k] = (float)g3[k];
  m.tolerance = (float)B.D1("opt_tolerance"); m.ls_tolerance = (float)B.D1("opt_ls_tolerance");
  m.impratio = (float)B.D1("opt_impratio"); m.meaninertia = (float)B.D1("stat_meaninertia");
  B.I("opt_iterations", &m.iterations, 1); B.I("opt_ls_iterations", &m.ls_iterations, 1);
  B.I("opt_eulerdamp", &c.eulerdamp, 1);
  return 0;
}

// <equality> (mjcf.py compiles joint / connect / weld; the float64 oracle builds all their rows).  The kernels model <equality><joint>
// rows between two hinges of one serial chain (odk_kernels.h "equality rows": shapes with S::EQ, at most EQ_MAX rows, a dof in at most
// one); every other ACTIVE equality is refused by name instead of being stepped without it.  Collected here, finished in
// load_equalities once the reduced layout and the shape are known.
int collect_equalities(Load& c) {
  Blob& B = c.B;
  const Blob::Rec* et = B.find("eq_type");
  if (!et || et->h.nbytes == 0) return 0;   // optional: a model without <equality>
  const int n = c.eq_n = B.optI("eq_type", c.eq_type, 16);
  if (n < 0 || B.optI("eq_active", c.eq_active, 16) != n || B.optI("eq_obj1id", c.eq_o1, 16) != n || B.optI("eq_obj2id", c.eq_o2, 16) != n ||
      B.optD("eq_data", c.eq_data, 16 * 11) != 11 * n || B.optD("eq_solref", c.eq_solref, 32) != 2 * n || B.optD("eq_solimp", c.eq_solimp, 80) != 5 * n)
    return fail(ODK_ERR_UNSUPPORTED, "equality constraints: more than 16, or eq_* records incomplete");
  for (int k = 0; k < n; k++)
    if (c.eq_active[k] && (c.eq_type[k] < 0 || c.eq_type[k] > 2)) return fail(ODK_ERR_UNSUPPORTED, "<equality> constraint %d: type %d (connect, weld and joint are modelled)", k, c.eq_type[k]);
  return 0;
}

// bodies / joints / dofs: the tree and its topology tables (tables.py), copied
int load_tree(Load& c) {
  Blob& B = c.B; DevModel& m = c.m;
  // bodies
  B.I("k_base_body", &m.base_body, 1); B.I("k_body_in_tree", m.body_in_tree, MAXB); B.I("body_parentid", m.body_parent, MAXB);
  B.I("body_jntadr", m.body_jntadr, MAXB); B.I("body_jntnum", m.body_jntnum, MAXB);
  B.I2("k_body_chain", &m.body_chain[0][0], MAXB, MAXCHAIN); B.I("k_body_chain_len", m.body_chain_len, MAXB);
  B.I2("k_body_ancdof", &m.body_ancdof[0][0], MAXB, MAXV); B.I("k_body_nancdof", m.body_nancdof, MAXB);
  B.I2("k_body_sub", &m.body_sub[0][0], MAXB, MAXB); B.I("k_body_nsub", m.body_nsub, MAXB);
  B.I("k_max_level", &m.max_level, 1); B.I("k_body_level", m.body_level, MAXB);
  for (int b2 = 0; b2 < MAXB; b2++) for (int k = 0; k < 4; k++) m.body_children[b2][k] = -1;   // (a blob with three columns: no fourth child)
  B.I2("k_body_children", &m.body_children[0][0], MAXB, 4);
  B.I("k_max_nonpath_level", &m.max_nonpath_level, 1); B.I("k_body_pathmask", m.body_pathmask, MAXB); B.I("k_body_is_path", m.body_is_path, MAXB);
  B.I("k_body_upmask", m.body_upmask, MAXB); B.I("k_body_path_head", m.body_path_head, MAXB);
  B.F("body_pos", &m.body_pos[0][0], MAXB * 3); B.F("body_quat", &m.body_quat[0][0], MAXB * 4); B.F("body_ipos", &m.body_ipos[0][0], MAXB * 3);
  B.F("body_mass", m.body_mass, MAXB); B.F("body_inertia_full", &m.body_inertia[0][0], MAXB * 6);
  // joints
  B.I("jnt_qposadr", m.jnt_qposadr, MAXJ); B.I("jnt_dofadr", m.jnt_dofadr, MAXJ); B.I("jnt_bodyid", m.jnt_bodyid, MAXJ);
  B.F("jnt_axis", &m.jnt_axis[0][0], MAXJ * 3); B.F("jnt_pos", &m.jnt_pos[0][0], MAXJ * 3); B.F("jnt_range", &m.jnt_range[0][0], MAXJ * 2);
  B.F("qpos0", m.qpos0, MAXQ); B.F("key_qpos", m.key_qpos, MAXQ); B.F("key_ctrl", m.key_ctrl, MAXU);
  // dofs
  B.I("dof_bodyid", m.dof_body, MAXV); B.I("k_dof_depth", m.dof_depth, MAXV); B.I2("k_dof_anc", &m.dof_anc[0][0], MAXV, MAXV);
  B.I("k_dof_Madr", m.dof_Madr, MAXV); B.I2("k_dof_anc_adr", &m.dof_anc_adr[0][0], MAXV, MAXV);
  B.I("k_dof_ndesc", m.dof_ndesc, MAXV); B.I2("k_dof_desc", &m.dof_desc[0][0], MAXV, MAXV); B.I2("k_dof_desc_adr", &m.dof_desc_adr[0][0], MAXV, MAXV);
  B.I("k_dof_nprefix", m.dof_nprefix, MAXV); B.I2("k_dof_prefix", &m.dof_prefix[0][0], MAXV, MAXV);
  B.I("k_dof_nsym", m.dof_nsym, MAXV); B.I2("k_dof_sym_dof", &m.dof_sym_dof[0][0], MAXV, MAXV); B.I2("k_dof_sym_adr", &m.dof_sym_adr[0][0], MAXV, MAXV);
  B.I("k_dof_act", m.dof_act, MAXV); B.I("k_dof_flrow", m.dof_flrow, MAXV); B.I("k_dof_limrow", m.dof_limrow, MAXV);
  B.I("k_dof_ancmask", m.dof_ancmask, MAXV); B.I("k_dof_descmask", m.dof_descmask, MAXV);
  B.I("k_vdof_ancmask", m.vdof_ancmask, MAXV); B.I("k_vdof_descmask", m.vdof_descmask, MAXV);
  B.F("dof_armature", m.dof_armature, MAXV); B.F("dof_damping", m.dof_damping, MAXV); B.F("dof_frictionloss", m.dof_frictionloss, MAXV);
  B.F("dof_invweight0", m.dof_invweight0, MAXV);
  B.I("k_nM", &m.nM, 1); B.I("k_M_i", m.M_i, MAXNZ); B.I("k_M_j", m.M_j, MAXNZ);
  for (int d = 0; d < MAXV; d++) { m.dof_qadr[d] = -1; m.dof_jnt[d] = -1; }
  for (int j = 1; j < m.nj; j++) {
    const int d = m.jnt_dofadr[j];
    m.dof_qadr[d] = m.jnt_qposadr[j]; m.dof_jnt[d] = j;
    m.dof_range[d][0] = m.jnt_range[j][0]; m.dof_range[d][1] = m.jnt_range[j][1];
    if (m.jnt_pos[j][0] != 0.0f || m.jnt_pos[j][1] != 0.0f || m.jnt_pos[j][2] != 0.0f) return fail(ODK_ERR_UNSUPPORTED, "hinge joints must sit at their body origin (jnt_pos == 0)");
  }
  for (int b2 = 0; b2 < m.nb; b2++) if (m.body_jntnum[b2] > 2) return fail(ODK_ERR_UNSUPPORTED, "more than two joints on one body");
  memset(c.body_name, 0, sizeof(c.body_name));
  c.has_names = B.optI("k_body_name", &c.body_name[0][0], MAXB * 32) == m.nb * 32;
  // Two hinges on one body are a joint and its backlash twin (same axis: build_reduced_tables) and nothing else: only the twin shape's
  // kernels carry a second joint slot (Shape::MAXJB), so two independent hinges on one body are refused here, by the body's name
  for (int b2 = 0; b2 < m.nb; b2++) {
    if (b2 == m.base_body || m.body_jntnum[b2] != 2) continue;
    const int j0 = m.body_jntadr[b2], j1 = j0 + 1;
    if (j0 < 1 || j1 >= m.nj) return fail(ODK_ERR_INVALID, "body_jntadr of %s", body_label(c, b2).c_str());
    if (m.jnt_axis[j0][0] != m.jnt_axis[j1][0] || m.jnt_axis[j0][1] != m.jnt_axis[j1][1] || m.jnt_axis[j0][2] != m.jnt_axis[j1][2])
      return fail(ODK_ERR_UNSUPPORTED, "%s carries two hinge joints that are not a joint and its backlash twin: the kernels take one hinge per body (give the second hinge a body of its own)",
                  body_label(c, b2).c_str());
  }
  B.I("k_vdof_depth", m.vdof_depth, MAXV); B.I2("k_vdof_anc", &m.vdof_anc[0][0], MAXV, MAXV); B.I("k_vdof_Madr", m.vdof_Madr, MAXV);
  B.I2("k_vdof_anc_adr", &m.vdof_anc_adr[0][0], MAXV, MAXV); B.I("k_vdof_ndesc", m.vdof_ndesc, MAXV);
  B.I2("k_vdof_desc", &m.vdof_desc[0][0], MAXV, MAXV); B.I2("k_vdof_desc_adr", &m.vdof_desc_adr[0][0], MAXV, MAXV);
  B.I("k_nH", &m.nH, 1); B.I("k_H_i", m.H_i, MAXNZ); B.I("k_H_j", m.H_j, MAXNZ); B.I("k_H_src", m.H_src, MAXNZ);
  B.I("k_tri_m", m.tri_m, MAXNZ); B.I("k_tri_q", m.tri_q, MAXNZ);
  return 0;
}

int load_actuators(Load& c) {
  Blob& B = c.B; DevModel& m = c.m;
  B.I("k_act_qposadr", m.act_qposadr, MAXU); B.I("k_act_dofadr", m.act_dofadr, MAXU); B.I("k_act_backlash_qposadr", m.act_backlash_qposadr, MAXU);
  B.F("actuator_gainprm0", m.act_kp, MAXU);
  float bias[MAXU * 3], gear[MAXU];
  B.F("actuator_biasprm", bias, MAXU * 3); B.F("actuator_gear", gear, MAXU);
  for (int u = 0; u < m.nu; u++) {
    m.act_bias1[u] = bias[3 * u + 1]; m.act_bias2[u] = bias[3 * u + 2];
    if (bias[3 * u] != 0.0f || gear[u] != 1.0f || fabsf(bias[3 * u + 1] + m.act_kp[u]) > 1e-6f) return fail(ODK_ERR_UNSUPPORTED, "only gear-1 position actuators are supported");
  }
  B.F("actuator_ctrlrange", &m.act_ctrlrange[0][0], MAXU * 2); B.F("actuator_forcerange", &m.act_forcerange[0][0], MAXU * 2);
  B.I("actuator_ctrllimited", m.act_ctrllimited, MAXU); B.I("actuator_forcelimited", m.act_forcelimited, MAXU);
  return 0;
}

// friction-loss and joint-limit rows
int load_rows(Load& c) {
  Blob& B = c.B; DevModel& m = c.m;
  m.nfl = B.I("k_fl_dof", m.fl_dof, MAXV); m.nlim = B.I("k_lim_jnt", m.lim_jnt, MAXJ);
  if (!B.ok) return missing(c);
  m.nrow = m.nfl + m.nlim + 48;
  double dof_solref[MAXV * 2], dof_solimp[MAXV * 5], jnt_solref[MAXJ * 2], jnt_solimp[MAXJ * 5], jnt_margin[MAXJ];
  B.D("dof_solref", dof_solref, MAXV * 2); B.D("dof_solimp", dof_solimp, MAXV * 5); B.D("dof_invweight0", c.dof_iw, MAXV);
  B.D("jnt_solref", jnt_solref, MAXJ * 2); B.D("jnt_solimp", jnt_solimp, MAXJ * 5); B.D("jnt_margin", jnt_margin, MAXJ);
  for (int r = 0; r < m.nfl; r++) {
    int d = m.fl_dof[r];
    double R, bb;
    row_consts(dof_solref + 2 * d, dof_solimp + 5 * d, c.dt, c.dof_iw[d], &R, &bb);
    m.fl_R[r] = (float)R; m.fl_D[r] = (float)(1.0 / R); m.fl_b[r] = (float)bb;
  }
  for (int r = 0; r < m.nlim; r++) {
    int j = m.lim_jnt[r];
    if (jnt_margin[j] != 0) return fail(ODK_ERR_UNSUPPORTED, "joint margin");
    for (int k = 0; k < 2; k++) m.lim_solref[r][k] = (float)jnt_solref[2 * j + k];
    for (int k = 0; k < 5; k++) m.lim_solimp[r][k] = (float)jnt_solimp[5 * j + k];
    pack_imp(m.lim_solref[r], m.lim_solimp[r], m.dt, m.lim_imp[r]);
    m.lim_invweight[r] = (float)c.dof_iw[m.jnt_dofadr[j]];
  }
  return 0;
}

// collision geoms: the two foot colliders (hull tables, or a sphere / capsule)
int load_feet(Load& c) {
  Blob& B = c.B; DevModel& m = c.m;
  int cg_vadr[4], cg_vnum[4], cg_fadr[4], cg_fnum[4], cg_condim[4], hf[128 * 3];
  double hv[64 * 3];
  B.I("k_foot_cgeom", c.foot_cg, 2); B.I("k_floor_cgeom", &c.floor_cg, 1); const int ncg = B.I("cgeom_type", c.cg_type, 4);
  B.I("cgeom_bodyid", c.cg_body, 4); B.I("cgeom_priority", c.cg_prio, 4); B.I("cgeom_condim", cg_condim, 4);
  B.I("cgeom_vertadr", cg_vadr, 4); B.I("cgeom_vertnum", cg_vnum, 4); B.I("cgeom_faceadr", cg_fadr, 4); B.I("cgeom_facenum", cg_fnum, 4);
  B.D("cgeom_pos", c.cg_pos, 12); B.D("cgeom_quat", c.cg_quat, 16); B.D("cgeom_friction", c.cg_fric, 12);
  B.D("cgeom_solref", c.cg_solref, 8); B.D("cgeom_solimp", c.cg_solimp, 20); B.D("cgeom_solmix", c.cg_solmix, 4);
  double cg_size[12] = {0}, cg_margin[4] = {0};
  B.optD("cgeom_size", cg_size, 12);       // optional: absent in blobs without primitive colliders
  B.optD("cgeom_margin", cg_margin, 4);    // optional: blobs of rounds 1-3 have none (= 0)
  B.D("hull_vert", hv, 64 * 3); B.I("hull_face", hf, 128 * 3);
  B.D("body_invweight0", c.biw, MAXB * 2);
  B.I("k_foot_body", m.foot_body, 2); B.I2("k_foot_dofmask", &m.foot_dofmask[0][0], 2, MAXV);
  for (int p = 0; p < m.nM && p < MAXNZ; p++) {
    const int i = m.M_i[p], j = m.M_j[p];
    const int fi = m.foot_dofmask[0][i] | (m.foot_dofmask[1][i] << 1), fj = m.foot_dofmask[0][j] | (m.foot_dofmask[1][j] << 1);
    m.M_ent[p] = i | (j << 5) | (fi << 10) | (fj << 12);
  }
  if (!B.ok || ncg != 3) return missing(c);
  const int* foot_cg = c.foot_cg; const int* cg_type = c.cg_type; const double* cg_pos = c.cg_pos;
  {   // the kernels' pair structure is fixed: floor x left foot, floor x right foot, left foot x right foot.  MuJoCo collides geoms g1, g2 when
      // (contype1 & conaffinity2) || (contype2 & conaffinity1): a model whose masks leave one of the three out would get a pair it does not have
    int ct[4] = {1, 1, 1, 1}, ca[4] = {1, 1, 1, 1};
    B.optI("cgeom_contype", ct, 4); B.optI("cgeom_conaffinity", ca, 4);   // optional: without them every geom collides with every other
    auto collide = [&](int g1, int g2) { return ((ct[g1] & ca[g2]) | (ct[g2] & ca[g1])) != 0; };
    if (!collide(c.floor_cg, foot_cg[0]) || !collide(c.floor_cg, foot_cg[1]) || !collide(foot_cg[0], foot_cg[1]))
      return fail(ODK_ERR_UNSUPPORTED, "contype / conaffinity exclude one of the three geom pairs the kernels collide (floor x each foot, foot x foot)");
  }
  for (int g = 0; g < 3; g++)   // the culls (height-field prisms, foot-foot boxes) drop every pair with a positive gap: only valid at margin 0
    if (cg_margin[g] != 0) return fail(ODK_ERR_UNSUPPORTED, "collision geom %d has margin %g: contacts are detected at distance 0", g, cg_margin[g]);
  m.foot_prim = 0;
  for (int f = 0; f < 2; f++) {
    int g = foot_cg[f];
    if (cg_condim[g] != 3) return fail(ODK_ERR_UNSUPPORTED, "foot collider condim %d: the contact rows are pyramidal condim-3", cg_condim[g]);
    if (cg_vnum[g] > HULL_MAXV || cg_fnum[g] > MAXHF)
      return fail(ODK_ERR_UNSUPPORTED, "foot hull with %d vertices / %d triangles: the kernels hold <= %d vertices and <= %d merged faces", cg_vnum[g], cg_fnum[g], HULL_MAXV, HULL_MAXF);
    double gm[9];
    quat2mat(c.cg_quat + 4 * g, gm);
    m.foot_gtype[f] = cg_type[g];
    for (int k = 0; k < 3; k++) { m.foot_gpos[f][k] = (float)cg_pos[3 * g + k]; m.foot_gaxis[f][k] = (float)gm[3 * k + 2]; m.foot_gsize[f][k] = (float)cg_size[3 * g + k]; }
    if (cg_type[g] == 2 || cg_type[g] == 3) {   // sphere / capsule foot: no hull; bounding box for the records only
      if (!(cg_size[3 * g] > 0) || (cg_type[g] == 3 && !(cg_size[3 * g + 1] > 0))) return fail(ODK_ERR_INVALID, "primitive foot collider without a size");
      m.foot_prim = 1;
      m.foot_nvert[f] = 0; m.foot_nface[f] = 0; m.foot_npoly[f] = 0; m.foot_nedge[f] = 0;
      const double hz = cg_type[g] == 3 ? cg_size[3 * g] + cg_size[3 * g + 1] : cg_size[3 * g];
      m.foot_obb_half[f][0] = m.foot_obb_half[f][1] = (float)cg_size[3 * g]; m.foot_obb_half[f][2] = (float)hz;
      for (int k = 0; k < 3; k++) { m.foot_obb_center[f][k] = (float)cg_pos[3 * g + k]; m.foot_centroid[f][k] = (float)cg_pos[3 * g + k]; }
      for (int k = 0; k < 9; k++) m.foot_obb_axes[f][k] = (float)gm[k];
      continue;
    }
    if (cg_type[g] != 7) return fail(ODK_ERR_UNSUPPORTED, "foot collider must be a convex mesh / box hull, a sphere or a capsule");
    m.foot_nvert[f] = cg_vnum[g]; m.foot_nface[f] = cg_fnum[g];
    // the hull in the body frame, in double precision: the vertices (rounded for the kernels), and from them polygons / edges / normals
    double bv[MAXHV][3], lo[3] = {1e30, 1e30, 1e30}, hi[3] = {-1e30, -1e30, -1e30};
    int tr[MAXHF][3];
    for (int v = 0; v < cg_vnum[g]; v++) {
      const double* p = hv + 3 * (cg_vadr[g] + v);
      for (int k = 0; k < 3; k++) {
        bv[v][k] = cg_pos[3 * g + k] + gm[3 * k] * p[0] + gm[3 * k + 1] * p[1] + gm[3 * k + 2] * p[2];
        m.foot_vert[f][v][k] = (float)bv[v][k];
        lo[k] = fmin(lo[k], p[k]); hi[k] = fmax(hi[k], p[k]);
      }
    }
    for (int t = 0; t < cg_fnum[g]; t++) for (int k = 0; k < 3; k++) m.foot_face[f][t][k] = tr[t][k] = hf[3 * (cg_fadr[g] + t) + k];
    double cl[3];
    for (int k = 0; k < 3; k++) { cl[k] = 0.5 * (lo[k] + hi[k]); m.foot_obb_half[f][k] = (float)(0.5 * (hi[k] - lo[k])); }
    for (int k = 0; k < 3; k++) m.foot_obb_center[f][k] = (float)(cg_pos[3 * g + k] + gm[3 * k] * cl[0] + gm[3 * k + 1] * cl[1] + gm[3 * k + 2] * cl[2]);
    for (int k = 0; k < 9; k++) m.foot_obb_axes[f][k] = (float)gm[k];
    if (!build_convex_tables(bv, cg_vnum[g], tr, cg_fnum[g], &m.foot_npoly[f], m.foot_poly[f], m.foot_fnorm[f], &m.foot_nedge[f], m.foot_edge[f],
                             m.foot_centroid[f], HULL_MAXF, HULL_MAXE))
      return fail(ODK_ERR_UNSUPPORTED, "foot hull: not a closed polytope with <= 4-vertex faces, <= %d merged faces and <= %d edges", HULL_MAXF, HULL_MAXE);
    for (int j = 0; j < 16; j++) {   // what a row lane keeps in registers over the height-field pair loop, as ONE 32-byte record
      for (int sl = 0; sl < 3; sl++) {
        const int jb = j + 16 * sl; const bool on = jb < m.foot_nedge[f]; const int* e = m.foot_edge[f][on ? jb : 0];
        m.foot_lane_rec[f][j][sl] = (int)((unsigned)e[2] | (unsigned)e[3] << 8 | (unsigned)e[0] << 16 | (unsigned)e[1] << 24 | (on ? 0u : 0x80000000u));
      }
      for (int sl = 0; sl < 2; sl++) {
        const int t = j + 16 * sl; const bool on = t < m.foot_npoly[f]; const int* pl = m.foot_poly[f][on ? t : 0];
        m.foot_lane_rec[f][j][3 + sl] = (int)((unsigned)pl[0] | (unsigned)pl[1] << 3 | (unsigned)pl[2] << 8 | (unsigned)pl[3] << 13 | (unsigned)pl[4] << 18 | (on ? 0u : 0x80000000u));
      }
      for (int sl = 5; sl < 8; sl++) m.foot_lane_rec[f][j][sl] = 0;
    }
    for (int t = 0; t < m.foot_npoly[f]; t++) {
      const double* v0 = bv[m.foot_poly[f][t][1]];
      m.foot_foff[f][t] = (float)(m.foot_fnorm[f][t][0] * v0[0] + m.foot_fnorm[f][t][1] * v0[1] + m.foot_fnorm[f][t][2] * v0[2]);
    }
  }
  for (int f = 0; f < 2; f++) m.foot_sphere_r[f] = sqrtf(m.foot_obb_half[f][0] * m.foot_obb_half[f][0] + m.foot_obb_half[f][1] * m.foot_obb_half[f][1] + m.foot_obb_half[f][2] * m.foot_obb_half[f][2]);
  {   // a height-field prism's topology: the kernels' compile-time tables (odk_model.h) against this file's table builder
    const double pv[6][3] = {{0, 0, 1}, {1, 0, 1}, {0, 1, 1}, {0, 0, 0}, {1, 0, 0}, {0, 1, 0}};
    const int ptri[8][3] = {{0, 1, 2}, {3, 5, 4}, {0, 3, 4}, {0, 4, 1}, {1, 4, 5}, {1, 5, 2}, {2, 5, 3}, {2, 3, 0}};
    int np = 0, ne = 0, ppoly[5][5], pedge[9][4]; float fn[5][3], cc[3];
    bool same = build_convex_tables(pv, 6, ptri, 8, &np, ppoly, fn, &ne, pedge, cc, 5, 9) && np == 5 && ne == 9;
    for (int f = 0; same && f < 5; f++) for (int k = 0; k < 5; k++) same = same && ppoly[f][k] == PRISM_POLY[f][k];
    for (int k = 0; same && k < 9; k++) for (int t = 0; t < 4; t++) same = same && pedge[k][t] == PRISM_EDGE[k][t];
    if (!same) return fail(ODK_ERR_INVALID, "the kernels' compile-time prism tables disagree with build_convex_tables");
  }
  return 0;
}

// the floor (plane or height field) and the contact parameters of the three geom pairs
int load_floor(Load& c) {
  Blob& B = c.B; DevModel& m = c.m;
  const int g = c.floor_cg;
  m.floor_is_plane = c.cg_type[g] == 0;
  double pm[9];
  quat2mat(c.cg_quat + 4 * g, pm);
  // floor body is static at the world origin in every reference scene
  double n[3] = {pm[2], pm[5], pm[8]};
  for (int k = 0; k < 3; k++) { m.plane_pos[k] = (float)c.cg_pos[3 * g + k]; m.plane_n[k] = (float)n[k]; }
  make_frame_h(n, m.plane_frame);
  for (int k = 0; k < 9; k++) m.floor_mat[k] = (float)pm[k];
  if (!m.floor_is_plane) {   // height field samples + size (scene_rough_terrain_backlash.xml:22)
    double hs[4];
    if (!B.optF2("hfield_data", c.mo.hfield, &m.hfield_nrow, &m.hfield_ncol) || B.D("hfield_size", hs, 4) != 4) return fail(ODK_ERR_UNSUPPORTED, "height-field floor without hfield_data / hfield_size");
    for (int k = 0; k < 4; k++) m.hfield_size[k] = (float)hs[k];
    // hfield_contacts works on a window of <= 3 x 3 cells under the hull's oriented box (18 prisms per foot: the LIST region):
    // whatever the foot's orientation, its box must span less than two cells per axis (MJX sizes its sub-grid from the same
    // ratio at trace time; a finer field or a larger foot needs a larger window here, not silently dropped cells)
    if (m.hfield_nrow < 2 || m.hfield_ncol < 2) return fail(ODK_ERR_UNSUPPORTED, "height field smaller than 2 x 2 samples");
    if (m.foot_prim && !((m.foot_gtype[0] == 2 || m.foot_gtype[0] == 3) && (m.foot_gtype[1] == 2 || m.foot_gtype[1] == 3)))
      return fail(ODK_ERR_UNSUPPORTED, "height-field floor: both feet are hulls (hfield_convex) or both are spheres / capsules (hfield_sphere / hfield_capsule)");
    const double cell = fmin(2.0 * hs[0] / (m.hfield_ncol - 1), 2.0 * hs[1] / (m.hfield_nrow - 1));
    for (int f = 0; f < 2; f++) {
      const float* hh = m.foot_obb_half[f];
      const double diag = 2.0 * sqrt((double)hh[0] * hh[0] + (double)hh[1] * hh[1] + (double)hh[2] * hh[2]);
      if (!(diag < 2.0 * cell))
        return fail(ODK_ERR_UNSUPPORTED, "foot %d spans %.4f m, the height field's cells are %.4f m: the prism window holds feet smaller than two cells", f, diag, cell);
    }
  }
  // contact parameter mixing (mj_contactParam): pairs 0,1 = floor vs foot, pair 2 = foot vs foot
  const int* cg_prio = c.cg_prio; const double* cg_fric = c.cg_fric;
  for (int pr = 0; pr < 3; pr++) {
    int g1 = pr < 2 ? g : c.foot_cg[0], g2 = pr < 2 ? c.foot_cg[pr] : c.foot_cg[1];
    double mix;
    if (cg_prio[g1] > cg_prio[g2]) mix = 1; else if (cg_prio[g2] > cg_prio[g1]) mix = 0;
    else { double s1 = c.cg_solmix[g1], s2 = c.cg_solmix[g2]; mix = (s1 >= 1e-15 && s2 >= 1e-15) ? s1 / (s1 + s2) : ((s1 < 1e-15 && s2 < 1e-15) ? 0.5 : (s1 < 1e-15 ? 0.0 : 1.0)); }
    for (int k = 0; k < 2; k++) m.pair_solref[pr][k] = (float)(mix * c.cg_solref[2 * g1 + k] + (1 - mix) * c.cg_solref[2 * g2 + k]);
    for (int k = 0; k < 5; k++) m.pair_solimp[pr][k] = (float)(mix * c.cg_solimp[5 * g1 + k] + (1 - mix) * c.cg_solimp[5 * g2 + k]);
    pack_imp(m.pair_solref[pr], m.pair_solimp[pr], m.dt, m.pair_imp[pr]);
    double mu = cg_prio[g1] > cg_prio[g2] ? cg_fric[3 * g1] : (cg_prio[g2] > cg_prio[g1] ? cg_fric[3 * g2] : fmax(cg_fric[3 * g1], cg_fric[3 * g2]));
    m.pair_mu[pr] = (float)mu;
    double t = c.biw[2 * c.cg_body[g1]] + c.biw[2 * c.cg_body[g2]];
    // pyramidal rows: the pyramid edge's weight; elliptic cones: the two bodies' translational weights (the normal row's; the kernels scale the tangents)
    m.pair_invweight[pr] = m.cone ? (float)t : (float)((t + mu * mu * t) * 2 * mu * mu / (double)m.impratio);
  }
  return 0;
}

// sites / sensors
int load_sensors(Load& c) {
  Blob& B = c.B; DevModel& m = c.m;
  B.I("site_bodyid", m.site_body, MAXSITE); B.F("site_pos", &m.site_pos[0][0], MAXSITE * 3); B.F("site_quat", &m.site_quat[0][0], MAXSITE * 4);
  {
    double sq[MAXSITE * 4];
    B.D("site_quat", sq, MAXSITE * 4);
    for (int s = 0; s < m.nsite; s++) { double mm[9]; quat2mat(sq + 4 * s, mm); for (int k = 0; k < 9; k++) m.site_mat[s][k] = (float)mm[k]; }
  }
  B.I("k_site_imu", &m.site_imu, 1); B.I("k_site_feet", m.site_feet, 2);
  m.nsensor = B.I("sensor_type", m.sensor_type, MAXSENS); B.I("sensor_objid", m.sensor_site, MAXSENS); B.I("sensor_adr", m.sensor_adr, MAXSENS);
  int adr[7];
  B.I("k_adr", adr, 7);
  m.adr_gyro = adr[0]; m.adr_local_linvel = adr[1]; m.adr_accelerometer = adr[2]; m.adr_upvector = adr[3]; m.adr_global_angvel = adr[4];
  m.adr_foot_linvel[0] = adr[5]; m.adr_foot_linvel[1] = adr[6];
  B.optI("k_adr_global_linvel", &c.mo.adr_global_linvel, 1);   // optional: blobs written before the reward library have none (-1)
  const int nsd = B.I1("nsensordata");
  if (!B.ok) return missing(c);
  if (nsd != NSENSD) return fail(ODK_ERR_UNSUPPORTED, "sensordata size %d != %d", nsd, NSENSD);
  if (c.eulerdamp != 0 || m.iterations != 1) return fail(ODK_ERR_UNSUPPORTED, "kernels implement iterations=1, eulerdamp=disable (open_duck_mini_v2.xml:6-8)");
  for (int s = 0; s < m.nsensor; s++) {
    int b = m.site_body[m.sensor_site[s]];
    bool ok = (b == m.base_body) || (b == m.foot_body[0]) || (b == m.foot_body[1]);
    if (!ok || ((m.sensor_type[s] == 2 || m.sensor_type[s] == 8) && b != m.base_body)) return fail(ODK_ERR_UNSUPPORTED, "sensor %d placement", s);
  }
  return 0;
}

// bodies above the serial chains that have children: flattened source lists for the one-step subtree fold (P2)
int build_fold_lists(Load& c) {
  DevModel& m = c.m;
  m.np_count = 0;
  for (int b2 = 0; b2 < m.nb; b2++) {
    if (!(m.body_level[b2] >= 0 && m.body_children[b2][0] >= 0 && !m.body_is_path[b2])) continue;
    if (m.np_count == 4) return fail(ODK_ERR_UNSUPPORTED, "more than four branching bodies above the serial chains");
    const int i = m.np_count++;
    m.np_body[i] = b2; m.np_nsrc[i] = 0;
    for (int c2 = 0; c2 < m.nb; c2++) {   // c2 in the subtree of b2 (or b2 itself) and either not a chain body, or a chain head
      bool below = false;
      for (int a2 = c2; a2 > 0; a2 = m.body_parent[a2]) if (a2 == b2) { below = true; break; }
      if (!below || m.body_level[c2] < 0) continue;
      if (!m.body_is_path[c2] || m.body_path_head[c2]) {
        if (m.np_nsrc[i] == 6) return fail(ODK_ERR_UNSUPPORTED, "more than six sources in a subtree fold");
        m.np_src[i][m.np_nsrc[i]++] = c2;
      }
    }
  }
  return 0;
}

// the reduced (twins merged) tree, the body-to-lane layout and the compiled shape that takes the model
int select_shape(Load& c) {
  DevModel& m = c.m;
  if (!build_reduced_tables(m)) return fail(ODK_ERR_UNSUPPORTED, "dof tree is not a floating base with up to four serial chains of <= 6 (twin-merged) dofs");
  if (!fill_body_st(m)) return fail(ODK_ERR_UNSUPPORTED, "no body-to-lane layout: every serial body chain must fit in one 16-lane row and all %d bodies in 32 lanes", m.nb);
  int dt_max = 0, dv_max = 0;
  for (int d = 0; d < m.nv; d++) { dt_max = m.dof_depth[d] > dt_max ? m.dof_depth[d] : dt_max; dv_max = m.vdof_depth[d] > dv_max ? m.vdof_depth[d] : dv_max; }
  int shape = -1, shape_cl = 5, shape_nch = 3, shape_maxjb = 1;
#define X(i, S) if (shape < 0 && m.nq == S::NQ && m.nv == S::NV && m.nb == S::NB && m.nu == S::NU && m.nj == S::NJ && m.nM == S::NM && m.nH == S::NH && m.nrow == S::NROW && \
                    dt_max <= S::DT && dv_max <= S::DV) { shape = i; shape_cl = S::CL; shape_nch = S::NCH; shape_maxjb = S::MAXJB; c.shape_eq = S::EQ; }
  ODK_SHAPES(X)
#undef X
  c.mo.shape = shape;
  if (shape < 0)
    return fail(ODK_ERR_UNSUPPORTED, "model shape nq=%d nv=%d nb=%d nu=%d nj=%d nM=%d nH=%d nrow=%d depth=%d vdepth=%d has no compiled kernel (tools/new_shape.py <xml> prints the three lines to add to odk_shapes.h)",
                m.nq, m.nv, m.nb, m.nu, m.nj, m.nM, m.nH, m.nrow, dt_max, dv_max);
  for (int k = 0; k < m.nrchain; k++)
    if (m.rchain_len[k] > shape_cl) return fail(ODK_ERR_UNSUPPORTED, "a serial chain of %d (twin-merged) dofs: the kernels of this model shape solve chains of <= %d", m.rchain_len[k], shape_cl);
  for (int b = 0; b < m.nb; b++)      // (the joint slots fill_body_st gave the body's lane: bodies below the floating base)
    if (m.body_in_tree[b] && m.body_level[b] > 0 && m.body_jntnum[b] > shape_maxjb)
      return fail(ODK_ERR_UNSUPPORTED, "%s carries %d hinge joints: the kernels of this model shape take %d per body", body_label(c, b).c_str(), m.body_jntnum[b], shape_maxjb);
  if (m.nrchain > shape_nch) return fail(ODK_ERR_UNSUPPORTED, "%d serial chains below the floating base: the kernels of this model shape solve <= %d", m.nrchain, shape_nch);
  if (!m.floor_is_plane && shape != 1) return fail(ODK_ERR_UNSUPPORTED, "height-field floors are built for the backlash model only");
  if (m.cone && m.foot_prim != 0)
    return fail(ODK_ERR_UNSUPPORTED, "<option cone=\"elliptic\">: the elliptic-cone kernels are built for convex (box / mesh) feet, not sphere / capsule feet");
  return 0;
}

// equality rows of the kernels: joint couplings inside one serial chain of a shape compiled with them
int load_equalities(Load& c) {
  DevModel& m = c.m;
  const bool shape_ok = c.shape_eq && !m.paired;      // shapes compiled with the optional constraint code (Shape::EQ)
  m.neq = 0;
  for (int d = 0; d < MAXV; d++) m.dof_eqrow[d] = -1;
  // <equality><connect | weld>: "path rows" (odk_kernels.h) -- the two bodies on ONE root-to-leaf path of the tree, or body2 = the world,
  // so that the rows' J^T D J only touches entries the tree layout has; at most EQP_MAX constraints / EQP_ROWS rows.  In MJX's row order:
  // connects first, then welds.
  m.neqp = 0; m.eqp_nrow = 0; m.eqp_cross = 0;
  for (int d = 0; d < MAXV; d++) m.dof_eqp[d] = 0;
  for (int pass = 0; pass < 2; pass++)
    for (int k = 0; k < c.eq_n; k++) {
      if (!c.eq_active[k] || c.eq_type[k] != pass) continue;
      const char* kind = pass == 0 ? "connect" : "weld";
      const int nrow = pass == 0 ? 3 : 6;
      if (!shape_ok || m.neqp == EQP_MAX || m.eqp_nrow + nrow > EQP_ROWS)
        return fail(ODK_ERR_UNSUPPORTED, "<equality><%s> (constraint %d) is active: %s", kind, k,
                    shape_ok ? "the kernels hold at most two connect / weld constraints with nine rows in total" : NO_EQ_ROWS);
      const int q = m.neqp, b1 = c.eq_o1[k], b2 = c.eq_o2[k] < 0 ? 0 : c.eq_o2[k];
      if (b1 < 1 || b1 >= m.nb || b2 >= m.nb) return fail(ODK_ERR_UNSUPPORTED, "<equality><%s> (constraint %d): bad body ids", kind, k);
      // dofs above a body: the dofs of the body itself and of its ancestors
      unsigned above[2] = {0u, 0u};
      for (int s2 = 0; s2 < 2; s2++)
        for (int b = s2 ? b2 : b1; b > 0; b = m.body_parent[b])
          for (int d = 0; d < m.nv; d++) if (m.dof_body[d] == b) above[s2] |= 1u << d;
      if ((above[0] & above[1]) != above[0] && (above[0] & above[1]) != above[1]) {
        // two chains: a closed loop.  The virtual tree (the Hessian layout of an active foot-foot contact: second leg below the first foot)
        // has an entry for every pair of dofs of base + the two foot chains -- a loop between exactly those is taken, on that layout
        unsigned legs = 0x3Fu;
        for (int f = 0; f < 2; f++) for (int t = 0; t < m.foot_rchain_len[f]; t++) legs |= 1u << (m.foot_rchain_first[f] + t);
        if (((above[0] | above[1]) & ~legs) != 0u || m.paired)
          return fail(ODK_ERR_UNSUPPORTED, "<equality><%s> (constraint %d): the two bodies must lie on one root-to-leaf path of the tree (or body2 be the world), or on the two foot chains: another loop has no entries in the Hessian's layouts", kind, k);
        m.eqp_cross = 1;
      }
      for (int d = 0; d < m.nv; d++) m.dof_eqp[d] |= (((above[0] >> d) & 1) << (2 * q)) | (((above[1] >> d) & 1) << (2 * q + 1));
      const double* da = c.eq_data + 11 * k;
      for (int a = 0; a < 3; a++) { m.eqp_a1[q][a] = (float)(pass == 0 ? da[a] : da[3 + a]); m.eqp_a2[q][a] = (float)(pass == 0 ? da[3 + a] : da[a]); }
      for (int a = 0; a < 4; a++) m.eqp_relq[q][a] = pass == 0 ? (a == 0 ? 1.0f : 0.0f) : (float)da[6 + a];
      m.eqp_ts[q] = pass == 0 ? 0.0f : (float)da[10];
      eq_pack_imp(c, k, m.eqp_imp[q]);
      m.eqp_invw[q][0] = (float)(c.biw[2 * b1] + c.biw[2 * b2]); m.eqp_invw[q][1] = (float)(c.biw[2 * b1 + 1] + c.biw[2 * b2 + 1]);
      m.eqp_type[q] = pass; m.eqp_b1[q] = b1; m.eqp_b2[q] = b2; m.eqp_row0[q] = m.eqp_nrow;
      m.eqp_nrow += nrow; m.neqp++;
    }
  for (int k = 0; k < c.eq_n; k++) {
    if (!c.eq_active[k] || c.eq_type[k] != 2) continue;
    if (!shape_ok || m.neq == EQ_MAX)
      return fail(ODK_ERR_UNSUPPORTED, "<equality><joint> (constraint %d) is active: %s", k, shape_ok ? "the kernels hold at most two equality rows" : NO_EQ_ROWS);
    const int r = m.neq, j1 = c.eq_o1[k], j2 = c.eq_o2[k];
    if (j1 < 1 || j1 >= m.nj || j2 >= m.nj || j2 == 0 || j2 == j1) return fail(ODK_ERR_UNSUPPORTED, "<equality><joint> (constraint %d): hinge joints expected", k);
    const int d1 = m.jnt_dofadr[j1], d2 = j2 > 0 ? m.jnt_dofadr[j2] : -1;
    if (m.dof_eqrow[d1] >= 0 || (d2 >= 0 && m.dof_eqrow[d2] >= 0)) return fail(ODK_ERR_UNSUPPORTED, "<equality><joint> (constraint %d): a joint takes part in at most one equality row", k);
    m.eq_dof1[r] = d1; m.eq_dof2[r] = d2; m.eq_qadr1[r] = m.jnt_qposadr[j1]; m.eq_qadr2[r] = j2 > 0 ? m.jnt_qposadr[j2] : 0;
    m.eq_key[r] = -1;
    if (d2 >= 0) {      // the Hessian entry (d1, d2) must exist in the reduced tree layout: same serial chain
      for (int p = 0; p < m.nMr; p++) {
        const int e = m.R_ent[p], i = e & 31, j = (e >> 5) & 31;
        if ((i == d1 && j == d2) || (i == d2 && j == d1)) m.eq_key[r] = e & 0x3FF;
      }
      if (m.eq_key[r] < 0) return fail(ODK_ERR_UNSUPPORTED, "<equality><joint> (constraint %d): the two joints must lie on one serial chain (the coupling's Hessian term needs an entry of the tree layout)", k);
    }
    for (int a = 0; a < 5; a++) m.eq_poly[r][a] = (float)c.eq_data[11 * k + a];
    eq_pack_imp(c, k, m.eq_imp[r]);
    m.eq_invweight[r] = (float)(c.dof_iw[d1] + (d2 >= 0 ? c.dof_iw[d2] : 0.0));
    m.dof_eqrow[d1] = r; if (d2 >= 0) m.dof_eqrow[d2] = r;
    m.neq++;
  }
  return 0;
}

// per-lane statics of the kernels (LaneSt) and the observation gather table, by the chosen shape
int build_statics(Load& c) {
  DevModel& m = c.m;
  const int shape = c.mo.shape;
  if (shape == 1 && !(m.paired && m.nvr == ShapeB::NVR && m.nMr == ShapeB::NMR && m.nHr == ShapeB::NHR))
    return fail(ODK_ERR_UNSUPPORTED, "the 30-dof kernels expect backlash twins (same body, anchor and axis as their joint) over the 20-dof tree");
  if (shape != 1 && m.paired) return fail(ODK_ERR_UNSUPPORTED, "twin dofs in a model of the 20-dof shape");
  for (int lane = 0; lane < 64; lane++) {
    memset(&m.lane_st[lane], 0, sizeof(LaneSt));
#define X(i, S) if (shape == i) compute_statics<S>(m.lane_st[lane], &m, lane);
    ODK_SHAPES(X)
#undef X
  }
#define X(i, S) if (shape == i) build_obs_table<S>(m);
  ODK_SHAPES(X)
#undef X
  return 0;
}

// the launch-invariant values of the substep in their packed form (DevModel::hot_pk / np_rec / hot_f): a value that does not fit its field is refused by name
int pack_hot(Load& c) {
  DevModel& m = c.m;
  const struct { const HotField& f; int v; } fields[] = {
      {HOT_FOOT_BODY0, m.foot_body[0]},         {HOT_FOOT_BODY1, m.foot_body[1]},         {HOT_FOOT_NVERT0, m.foot_nvert[0]},     {HOT_FOOT_NVERT1, m.foot_nvert[1]},
      {HOT_RCHAIN_FIRST0, m.foot_rchain_first[0]}, {HOT_RCHAIN_FIRST1, m.foot_rchain_first[1]}, {HOT_RCHAIN_LEN0, m.foot_rchain_len[0]}, {HOT_RCHAIN_LEN1, m.foot_rchain_len[1]},
      {HOT_LS_ITERATIONS, m.ls_iterations},     {HOT_NP_LEVELS, m.max_nonpath_level + 1}, {HOT_NP_COUNT, m.np_count},             {HOT_FOOT_PRIM, m.foot_prim}};
  for (int k = 0; k < HOT_NPK; k++) m.hot_pk[k] = 0;
  for (const auto& e : fields) {
    const long long stored = (long long)e.v * e.f.scale;
    if (e.v < 0 || stored >= (1ll << e.f.bits))
      return fail(ODK_ERR_UNSUPPORTED, "%s = %d does not fit the %d-bit field the step kernels read it from (0 .. %d)", e.f.name, e.v, e.f.bits,
                  (int)(((1ll << e.f.bits) - 1) / e.f.scale));
    m.hot_pk[e.f.word] |= (int)((unsigned)stored << e.f.shift);
  }
  for (int lane = 0; lane < 64; lane++) {
    const int i = lane >> 4;
    unsigned r0 = 0, r1 = 0;
    if (i < m.np_count) {
      const int* s = m.np_src[i];      // (bodies: < MAXB = 20, so every byte offset is below 80)
      r0 = (unsigned)(s[0] * 4) | (unsigned)(s[1] * 4) << 8 | (unsigned)(s[2] * 4) << 16 | (unsigned)(s[3] * 4) << 24;
      r1 = (unsigned)(s[4] * 4) | (unsigned)(s[5] * 4) << 8 | (unsigned)(m.np_body[i] * 4) << 16 | (unsigned)m.np_nsrc[i] << 24;
    }
    m.np_rec[lane][0] = (int)r0; m.np_rec[lane][1] = (int)r1;
  }
  for (int f = 0; f < 2; f++) {
    for (int k = 0; k < 3; k++) m.hot_f[HOT_F_OBBC + 3 * f + k] = m.foot_obb_center[f][k];
    m.hot_f[HOT_F_SPHR + f] = m.foot_sphere_r[f];
  }
  for (int k = 0; k < 3; k++) { m.hot_f[HOT_F_PLN + k] = m.plane_n[k]; m.hot_f[HOT_F_PLP + k] = m.plane_pos[k]; }
  m.hot_f[HOT_F_TOL] = m.tolerance; m.hot_f[HOT_F_LSTOL] = m.ls_tolerance; m.hot_f[HOT_F_MEANI] = m.meaninertia;
  return 0;
}
}  // namespace

extern "C" int odk_model_hot_words(const odk_model* m, int* packed, int* fields) {
  if (!m || !packed || !fields) return fail(ODK_ERR_INVALID, "odk_model_hot_words: bad arguments");
  const DevModel& h = m->h;
  for (int k = 0; k < HOT_NPK; k++) packed[k] = h.hot_pk[k];
  const int v[12] = {h.foot_body[0], h.foot_body[1], h.foot_nvert[0], h.foot_nvert[1], h.foot_rchain_first[0], h.foot_rchain_first[1], h.foot_rchain_len[0], h.foot_rchain_len[1],
                     h.ls_iterations, h.max_nonpath_level, h.np_count, h.foot_prim};
  for (int k = 0; k < 12; k++) fields[k] = v[k];
  return ODK_OK;
}

extern "C" int odk_model_load(const void* blob, uint64_t len, odk_model** out) {
  if (!blob || !out || len < 16 || memcmp(blob, "ODKM", 4) != 0) return fail(ODK_ERR_INVALID, "odk_model_load: not an ODKM blob");
  Blob B;
  if (const char* bad = B.open((const unsigned char*)blob, len)) return fail(ODK_ERR_INVALID, "odk_model_load: record %d: %s", (int)B.recs.size(), bad);
  auto mo = std::make_unique<odk_model>();
  memset(&mo->h, 0, sizeof(mo->h));   // (padding too: the same blob always gives the same bytes)
  Load c{B, *mo, mo->h};
  int (*const stages[])(Load&) = {load_options, collect_equalities, load_tree,        load_actuators, load_rows,       load_feet,
                                  load_floor,   load_sensors,       build_fold_lists, select_shape,   load_equalities, build_statics,
                                  pack_hot};
  for (auto stage : stages)
    if (const int err = stage(c)) return err;
  *out = mo.release();
  return ODK_OK;
}
extern "C" void odk_model_free(odk_model* m) { delete m; }
extern "C" int odk_model_dims(const odk_model* m, int* nq, int* nv, int* nu, int* nbody) {
  if (!m) return fail(ODK_ERR_INVALID, "null model");
  if (nq) *nq = m->h.nq; if (nv) *nv = m->h.nv; if (nu) *nu = m->h.nu; if (nbody) *nbody = m->h.nb;
  return ODK_OK;
}
extern "C" int odk_model_obs_sizes(const odk_model* m, int env_kind, int* nobs, int* npriv) {
  if (!m) return fail(ODK_ERR_INVALID, "null model");
  obs_sizes_nu(m->h.nu, env_kind, nobs, npriv);
  return ODK_OK;
}
extern "C" int odk_model_reduced(const odk_model* m, int* paired, int* nvr, int* nMr, int* nHr, int* red_main, int* red_twin) {
  if (!m) return fail(ODK_ERR_INVALID, "null model");
  if (paired) *paired = m->h.paired; if (nvr) *nvr = m->h.nvr; if (nMr) *nMr = m->h.nMr; if (nHr) *nHr = m->h.nHr;
  for (int r = 0; r < m->h.nvr; r++) { if (red_main) red_main[r] = m->h.red_main[r]; if (red_twin) red_twin[r] = m->h.red_twin[r]; }
  return ODK_OK;
}
extern "C" int odk_model_body_lanes(const odk_model* m, int lanes_per_env, int* out, int n) {
  if (!m || !out || (lanes_per_env != 32 && lanes_per_env != 64)) return fail(ODK_ERR_INVALID, "odk_model_body_lanes: bad arguments");
  for (int l = 0; l < n && l < lanes_per_env; l++) out[l] = m->h.body_st[lanes_per_env == 64][l].body;
  return ODK_OK;
}
extern "C" int odk_model_env_lds_floats(const odk_model* m) {
  if (!m) return -1;
#define X(i, S) if (m->shape == i) return EnvL<S>::TOTAL;
  ODK_SHAPES(X)
#undef X
  return -1;
}
