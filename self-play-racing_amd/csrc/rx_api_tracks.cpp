// rx_api_tracks.cpp -- C ABI (include/rx.h): the track table builders, the culling tables, slots
// patched in place and the rasteriser, each with its host twin.  Nothing here reads a handle; the
// handle's side (rx_upload_tracks_device, rx_replace_tracks_device) is in rx_api.cpp.
#include <cmath>

#include "rx_handle.h"
#include "rx_spline.h"

// ---- culling tables (csrc/rx_cull.h) ------------------------------------------
// What the host can check of a culling-table build, and the offsets: off receives
// wp_off and the chunk / super / wchunk / wsuper offset arrays back to back
// (n + 1 entries each), tot the four box totals.  sizes_only: the offsets alone are
// checked (rx_cull_table_sizes; rx_upload_tracks_device, whose arrays are the handle's).
int cull_check(const char* fn, int32_t n, const int32_t* wp_off, const void* wp, const void* seg, const void* meta,
               int32_t G, int32_t SG, const rx_cull_tables* out, bool sizes_only, std::vector<int32_t>* off,
               int64_t tot[4]) {
  if (n <= 0) return fail(RX_EINVAL, "%s: n_tracks must be > 0 (got %d)", fn, n);
  if (!wp_off) return fail(RX_EINVAL, "%s: wp_off is null", fn);
  if (!sizes_only) {
    if (!wp) return fail(RX_EINVAL, "%s: wp is null", fn);
    if (!seg) return fail(RX_EINVAL, "%s: seg is null", fn);
    if (!meta) return fail(RX_EINVAL, "%s: meta is null", fn);
    if (!out) return fail(RX_EINVAL, "%s: out is null", fn);
    const struct {
      const void* p;
      const char* name;
      bool need;
    } fields[] = {{out->seg_f, "seg_f", true},
                  {out->slot_hdr, "slot_hdr", true},
                  {out->chunk_off, "chunk_off", G > 0},
                  {out->wchunk_off, "wchunk_off", G > 0},
                  {out->wsuper_off, "wsuper_off", G > 0},
                  {out->chunk_box, "chunk_box", G > 0},
                  {out->wchunk_box, "wchunk_box", G > 0},
                  {out->wsuper_box, "wsuper_box", G > 0},
                  {out->slot_geo, "slot_geo", G > 0},
                  {out->chunk_box_f, "chunk_box_f", G > 0},
                  {out->super_off, "super_off", G > 0 && SG > 0},
                  {out->super_box, "super_box", G > 0 && SG > 0},
                  {out->super_box_f, "super_box_f", G > 0 && SG > 0}};
    for (const auto& f : fields)
      if (f.need && !f.p) return fail(RX_EINVAL, "%s: out->%s is null", fn, f.name);
  }
  if (SG < 0 || SG > RX_CULL_MAX_SUPER)
    return fail(RX_EINVAL, "%s: cull_super must be 0 .. %d (got %d)", fn, RX_CULL_MAX_SUPER, SG);
  if (wp_off[0] != 0) return fail(RX_EINVAL, "%s: wp_off[0] must be 0 (got %d)", fn, wp_off[0]);
  const size_t n1 = (size_t)n + 1;
  if (off) off->assign(5 * n1, 0);
  int64_t run[4] = {0, 0, 0, 0};
  for (int32_t k = 0; k < n; ++k) {
    const int64_t W = (int64_t)wp_off[k + 1] - wp_off[k];
    if (W < 2) return fail(RX_EINVAL, "%s: track %d has W = %lld waypoints (need >= 2)", fn, k, (long long)W);
    if (W > RX_CULL_MAX_W)
      return fail(RX_EINVAL, "%s: track %d has W = %lld waypoints (at most %d)", fn, k, (long long)W, RX_CULL_MAX_W);
    const rx_cull_counts c = rx_cull_slot_counts((int32_t)W, G, SG);
    const int32_t add[4] = {c.leaf, c.super, c.wchunk, c.wsuper};
    for (int a = 0; a < 4; ++a) {
      run[a] += add[a];
      if (run[a] > INT32_MAX)
        return fail(RX_EINVAL, "%s: track %d: the box count overflows the int32 offsets", fn, k);
      if (off) (*off)[(a + 1) * n1 + k + 1] = (int32_t)run[a];
    }
    if (off) (*off)[k + 1] = wp_off[k + 1];
  }
  for (int a = 0; a < 4; ++a) tot[a] = run[a];
  return RX_OK;
}

// ---- track table builders (ABI v24) ------------------------------------------
// What the host can check from the offsets alone; fills wp_off.
static int tracks_shape(const char* fn, int32_t n, int32_t factor, const int32_t* cp_off, const void* cp,
                        const void* width, int32_t* wp_off, const void* wp, const void* nrm, const void* seg,
                        const void* meta) {
  if (n <= 0) return fail(RX_EINVAL, "%s: n_tracks must be > 0 (got %d)", fn, n);
  if (!cp_off || !cp || !width || !wp_off || !wp || !nrm || !seg || !meta) return fail(RX_EINVAL, "%s: null buffer", fn);
  if (factor < 1) return fail(RX_EINVAL, "%s: factor must be >= 1 (got %d)", fn, factor);
  if (cp_off[0] != 0) return fail(RX_EINVAL, "%s: cp_off[0] must be 0", fn);
  const int max_w = 64 * RX_WP_CHUNK * RX_WP_SUPER;  // rx_upload_tracks' limit
  for (int32_t k = 0; k < n; ++k) {
    const int64_t P = (int64_t)cp_off[k + 1] - cp_off[k];
    if (P < 3 || P > RX_TRACK_MAX_P)
      return fail(RX_EINVAL, "%s: track %d has P = %lld control points (3 .. %d)", fn, k, (long long)P, RX_TRACK_MAX_P);
    if (P * factor > max_w)
      return fail(RX_EINVAL, "%s: track %d has W = P * factor = %lld waypoints (at most %d)", fn, k,
                  (long long)(P * factor), max_w);
  }
  if ((int64_t)cp_off[n] * factor > INT32_MAX)
    return fail(RX_EINVAL, "%s: W summed over the tracks = %lld overflows wp_off (int32)", fn,
                (long long)cp_off[n] * factor);
  for (int32_t k = 0; k <= n; ++k) wp_off[k] = cp_off[k] * factor;
  return RX_OK;
}

int rx_build_tracks(int32_t n, int32_t factor, const int32_t* cp_off, const double* cp, const double* width,
                    int32_t* wp_off, double* wp, double* nrm, double* seg, double* meta, void* stream) {
  const int rc = tracks_shape("rx_build_tracks", n, factor, cp_off, cp, width, wp_off, wp, nrm, seg, meta);
  if (rc != RX_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  int32_t* off_dev = nullptr;
  const size_t bytes = ((size_t)n + 1) * sizeof(int32_t);
  if (hipMallocAsync((void**)&off_dev, bytes, s) != hipSuccess || !off_dev)
    return fail(RX_ENOMEM, "rx_build_tracks: hipMallocAsync(%zu bytes) failed", bytes);
  hipError_t e = hipMemcpyAsync(off_dev, cp_off, bytes, hipMemcpyHostToDevice, s);
  int lrc = 0;
  if (e == hipSuccess) lrc = rx_launch_build_tracks(n, factor, off_dev, cp, width, wp, nrm, seg, meta, s);
  const hipError_t ef = hipFreeAsync(off_dev, s);
  if (e != hipSuccess) return fail(RX_EHIP, "rx_build_tracks: offset copy failed: %s", hipGetErrorString(e));
  if (lrc != 0) return launched("rx_build_tracks", lrc);
  if (ef != hipSuccess) return fail(RX_EHIP, "rx_build_tracks: hipFreeAsync failed: %s", hipGetErrorString(ef));
  return RX_OK;
}

int rx_build_tracks_host(int32_t n, int32_t factor, const int32_t* cp_off, const double* cp, const double* width,
                         int32_t* wp_off, double* wp, double* nrm, double* seg, double* meta, void* /*stream*/) {
  const int rc = tracks_shape("rx_build_tracks_host", n, factor, cp_off, cp, width, wp_off, wp, nrm, seg, meta);
  if (rc != RX_OK) return rc;
  for (int32_t k = 0; k < n; ++k) {  // the data, before anything is written
    const int P = cp_off[k + 1] - cp_off[k];
    int at = 0;
    switch (rx_track_check(P, cp + 2 * (size_t)cp_off[k], width[k], &at)) {
      case RX_TRACK_BAD_COORD:
        return fail(RX_EINVAL, "rx_build_tracks_host: track %d: cp[%d] has a non-finite coordinate", k, at);
      case RX_TRACK_BAD_CHORD:
        return fail(RX_EINVAL, "rx_build_tracks_host: track %d: chord %d (cp[%d] to cp[%d]) has zero or non-finite "
                               "length", k, at, at, (at + 1) % P);
      case RX_TRACK_BAD_WIDTH:
        return fail(RX_EINVAL, "rx_build_tracks_host: track %d: width %g is negative or NaN", k, width[k]);
      default:
        break;
    }
  }
  rx_spline_ws ws;
  for (int32_t k = 0; k < n; ++k) {  // the kernel's steps (rx_track.hip), one lane at a time
    const int P = cp_off[k + 1] - cp_off[k], W = P * factor;
    const double* c = cp + 2 * (size_t)cp_off[k];
    const size_t base = (size_t)wp_off[k];
    for (int i = 0; i < P; ++i) rx_spline_load(i, c, &ws);
    rx_spline_knots(P, W, &ws);
    rx_spline_solve(P, 0, &ws);
    rx_spline_solve(P, 1, &ws);
    for (int i = 0; i < P; ++i) rx_spline_coef(P, i, &ws);
    double b[4] = {HUGE_VAL, -HUGE_VAL, HUGE_VAL, -HUGE_VAL};
    for (int j = 0; j < W; ++j) {
      double x, y;
      rx_track_point(P, W, &ws, width[k], j, wp + 2 * base, nrm + 2 * base, seg + 8 * base, &x, &y);
      rx_track_bounds(x, y, b);
    }
    double dy, dx;
    rx_track_meta(P, W, &ws, width[k], b, meta + 8 * (size_t)k, &dy, &dx);
    meta[8 * (size_t)k + 2] = atan2(dy, dx);
  }
  return RX_OK;
}

// ---- culling tables (ABI v25, additive) -----------------------------------------
int rx_cull_table_sizes(int32_t n, const int32_t* wp_off, int32_t G, int32_t SG, int64_t* out) {
  if (!out) return fail(RX_EINVAL, "rx_cull_table_sizes: out is null");
  return cull_check("rx_cull_table_sizes", n, wp_off, nullptr, nullptr, nullptr, G, SG, nullptr, true, nullptr, out);
}

int rx_build_cull_tables_host(int32_t n, const int32_t* wp_off, const double* wp, const double* seg,
                              const double* meta, int32_t G, int32_t SG, const rx_cull_tables* t, void* /*stream*/) {
  std::vector<int32_t> off;
  int64_t tot[4];
  const int rc = cull_check("rx_build_cull_tables_host", n, wp_off, wp, seg, meta, G, SG, t, false, &off, tot);
  if (rc != RX_OK) return rc;
  const size_t n1 = (size_t)n + 1;
  for (int32_t k = 0; k < n; ++k) {  // the kernel's steps (rx_cull.hip) with one lane
    const int32_t wp0 = wp_off[k], W = wp_off[k + 1] - wp0;
    const double* s = seg + 8 * (size_t)wp0;
    rx_cull_slot o = {0, 0, 0, 0, tot[0], tot[1], t->chunk_box, t->super_box, t->wchunk_box, t->wsuper_box,
                      t->chunk_box_f, t->super_box_f};
    double b[4], longest, geo[4] = {0.0, 0.0, 0.0, 0.0};
    rx_cull_extent(s, W, 0, 1, t->seg_f + 8 * (size_t)wp0, b, &longest);
    if (G > 0) {
      rx_cull_geo(b, rx_cull_reach(s, W, 0, 1, 0.5 * (b[0] + b[2]), 0.5 * (b[1] + b[3])), longest, geo);
      o.chunk0 = off[n1 + k];
      o.super0 = SG > 0 ? off[2 * n1 + k] : 0;
      o.wchunk0 = off[3 * n1 + k];
      o.wsuper0 = off[4 * n1 + k];
      rx_cull_boxes(s, wp + 2 * (size_t)wp0, W, G, SG, 0, 1, &o);
      for (int c = 0; c < 4; ++c) t->slot_geo[4 * (size_t)k + c] = geo[c];
    }
    rx_cull_header((rx_slot_hdr*)t->slot_hdr + k, wp0, W, &o, geo, meta + 8 * (size_t)k);
  }
  if (G > 0) {
    std::copy(off.begin() + n1, off.begin() + 2 * n1, t->chunk_off);
    if (SG > 0) std::copy(off.begin() + 2 * n1, off.begin() + 3 * n1, t->super_off);
    std::copy(off.begin() + 3 * n1, off.begin() + 4 * n1, t->wchunk_off);
    std::copy(off.begin() + 4 * n1, off.begin() + 5 * n1, t->wsuper_off);
  }
  return RX_OK;
}

// The launch behind rx_build_cull_tables and rx_upload_tracks_device: `off` (cull_check's
// five offset arrays) goes up through a stream-ordered allocation, as rx_build_tracks'
// offsets do (a pageable source: the copy has left `off` when hipMemcpyAsync returns).
int cull_launch(const char* fn, int32_t n, const std::vector<int32_t>& off, const int64_t tot[4],
                       const double* wp, const double* seg, const double* meta, int32_t G, int32_t SG,
                       const rx_cull_tables* t, hipStream_t s) {
  int32_t* off_dev = nullptr;
  const size_t bytes = off.size() * sizeof(int32_t);
  if (hipMallocAsync((void**)&off_dev, bytes, s) != hipSuccess || !off_dev)
    return fail(RX_ENOMEM, "%s: hipMallocAsync(%zu bytes) failed", fn, bytes);
  hipError_t e = hipMemcpyAsync(off_dev, off.data(), bytes, hipMemcpyHostToDevice, s);
  int lrc = 0;
  if (e == hipSuccess) lrc = rx_launch_cull_tables(n, G, SG, off_dev, wp, seg, meta, t, tot[0], tot[1], s);
  const hipError_t ef = hipFreeAsync(off_dev, s);
  if (e != hipSuccess) return fail(RX_EHIP, "%s: offset copy failed: %s", fn, hipGetErrorString(e));
  if (lrc != 0) return launched(fn, lrc);
  if (ef != hipSuccess) return fail(RX_EHIP, "%s: hipFreeAsync failed: %s", fn, hipGetErrorString(ef));
  return RX_OK;
}

int rx_build_cull_tables(int32_t n, const int32_t* wp_off, const double* wp, const double* seg, const double* meta,
                         int32_t G, int32_t SG, const rx_cull_tables* t, void* stream) {
  std::vector<int32_t> off;
  int64_t tot[4];
  const int rc = cull_check("rx_build_cull_tables", n, wp_off, wp, seg, meta, G, SG, t, false, &off, tot);
  if (rc != RX_OK) return rc;
  return cull_launch("rx_build_cull_tables", n, off, tot, wp, seg, meta, G, SG, t, (hipStream_t)stream);
}


// ---- slots replaced in place (ABI v25, additive) ---------------------------------
// What the host can check of a patch, before any HIP call or write; ps receives the
// listed slots' rows for the kernel and the host twin, tot the table's box totals.
// t == nullptr: the four table arrays only (G and SG are then not looked at).
int patch_check(const char* fn, int32_t n, const int32_t* wp_off, const void* wp, const void* nrm,
                       const void* seg, const void* meta, int32_t G, int32_t SG, const rx_cull_tables* t,
                       const rx_track_patch* p, std::vector<rx_patch_slot>* ps, int64_t tot[4]) {
  if (n <= 0) return fail(RX_EINVAL, "%s: n_tracks must be > 0 (got %d)", fn, n);
  if (!wp_off) return fail(RX_EINVAL, "%s: wp_off is null", fn);
  if (!wp) return fail(RX_EINVAL, "%s: wp is null", fn);
  if (!nrm) return fail(RX_EINVAL, "%s: nrm is null", fn);
  if (!seg) return fail(RX_EINVAL, "%s: seg is null", fn);
  if (!meta) return fail(RX_EINVAL, "%s: meta is null", fn);
  if (!p) return fail(RX_EINVAL, "%s: the patch is null", fn);
  const struct {
    const void* q;
    const char* name;
  } fields[] = {{p->slots, "slots"}, {p->src_off, "src_off"}, {p->wp, "wp"},
                {p->nrm, "nrm"},     {p->seg, "seg"},         {p->meta, "meta"}};
  for (const auto& f : fields)
    if (!f.q) return fail(RX_EINVAL, "%s: patch->%s is null", fn, f.name);
  std::vector<int32_t> off;
  const int rc = t ? cull_check(fn, n, wp_off, wp, seg, meta, G, SG, t, false, &off, tot)
                   : cull_check(fn, n, wp_off, nullptr, nullptr, nullptr, 0, 0, nullptr, true, &off, tot);
  if (rc != RX_OK) return rc;
  if (p->n_upd < 1 || p->n_upd > n)
    return fail(RX_EINVAL, "%s: patch->n_upd must be 1 .. n_tracks = %d (got %d)", fn, n, p->n_upd);
  if (p->src_off[0] != 0) return fail(RX_EINVAL, "%s: patch->src_off[0] must be 0 (got %d)", fn, p->src_off[0]);
  const size_t n1 = (size_t)n + 1;
  ps->assign((size_t)p->n_upd, rx_patch_slot{});
  for (int32_t j = 0; j < p->n_upd; ++j) {
    const int32_t k = p->slots[j];
    if (k < 0 || k >= n)
      return fail(RX_EINVAL, "%s: patch->slots[%d] = slot %d is outside [0, %d)", fn, j, k, n);
    if (j > 0 && k <= p->slots[j - 1])
      return fail(RX_EINVAL, "%s: patch->slots[%d] = slot %d follows slot %d: the slots must be ascending and "
                             "distinct", fn, j, k, p->slots[j - 1]);
    const int64_t Ws = (int64_t)p->src_off[j + 1] - p->src_off[j], W = (int64_t)wp_off[k + 1] - wp_off[k];
    if (Ws != W)
      return fail(RX_EINVAL, "%s: slot %d: patch->src_off gives source track %d %lld waypoints, the slot has %lld "
                             "(a replaced slot keeps its waypoint count)", fn, k, j, (long long)Ws, (long long)W);
    (*ps)[j] = rx_patch_slot{k, p->src_off[j], wp_off[k], (int32_t)W, off[n1 + k], off[2 * n1 + k],
                             off[3 * n1 + k], off[4 * n1 + k]};
  }
  return RX_OK;
}

// rx_upload_tracks' per-track checks on the source meta rows (host memory), the slot named
int patch_check_meta(const char* fn, const rx_track_patch* p, const double* meta_h) {
  for (int32_t j = 0; j < p->n_upd; ++j) {
    const double* m = meta_h + 8 * (size_t)j;
    if (!(m[3] >= 0))
      return fail(RX_EINVAL, "%s: slot %d (source track %d): width %g is negative or NaN", fn, p->slots[j], j, m[3]);
    if (!(m[4] > 0))
      return fail(RX_EINVAL, "%s: slot %d (source track %d): max_track_distance must be > 0 (got %g; NaN marks a "
                             "track rx_build_tracks found invalid)", fn, p->slots[j], j, m[4]);
  }
  return RX_OK;
}

// The launch behind rx_patch_tracks and rx_replace_tracks_device: the listed slots' rows
// go up through a stream-ordered allocation, as cull_launch's offsets do.
int patch_launch(const char* fn, const std::vector<rx_patch_slot>& ps, const int64_t tot[4], double* wp,
                        double* nrm, double* seg, double* meta, int32_t G, int32_t SG, const rx_cull_tables* t,
                        const rx_track_patch* p, hipStream_t s) {
  rx_patch_slot* ps_dev = nullptr;
  const size_t bytes = ps.size() * sizeof(rx_patch_slot);
  if (hipMallocAsync((void**)&ps_dev, bytes, s) != hipSuccess || !ps_dev)
    return fail(RX_ENOMEM, "%s: hipMallocAsync(%zu bytes) failed", fn, bytes);
  hipError_t e = hipMemcpyAsync(ps_dev, ps.data(), bytes, hipMemcpyHostToDevice, s);
  int lrc = 0;
  if (e == hipSuccess)
    lrc = rx_launch_patch_slots((int)ps.size(), t ? G : 0, t ? SG : 0, ps_dev, p, wp, nrm, seg, meta, t, tot[0],
                                tot[1], s);
  const hipError_t ef = hipFreeAsync(ps_dev, s);
  if (e != hipSuccess) return fail(RX_EHIP, "%s: slot list copy failed: %s", fn, hipGetErrorString(e));
  if (lrc != 0) return launched(fn, lrc);
  if (ef != hipSuccess) return fail(RX_EHIP, "%s: hipFreeAsync failed: %s", fn, hipGetErrorString(ef));
  return RX_OK;
}

int rx_patch_tracks(int32_t n, const int32_t* wp_off, double* wp, double* nrm, double* seg, double* meta, int32_t G,
                    int32_t SG, const rx_cull_tables* t, const rx_track_patch* p, void* stream) {
  std::vector<rx_patch_slot> ps;
  int64_t tot[4];
  const int rc = patch_check("rx_patch_tracks", n, wp_off, wp, nrm, seg, meta, G, SG, t, p, &ps, tot);
  if (rc != RX_OK) return rc;
  return patch_launch("rx_patch_tracks", ps, tot, wp, nrm, seg, meta, G, SG, t, p, (hipStream_t)stream);
}

int rx_patch_tracks_host(int32_t n, const int32_t* wp_off, double* wp, double* nrm, double* seg, double* meta,
                         int32_t G, int32_t SG, const rx_cull_tables* t, const rx_track_patch* p, void* /*stream*/) {
  std::vector<rx_patch_slot> ps;
  int64_t tot[4];
  int rc = patch_check("rx_patch_tracks_host", n, wp_off, wp, nrm, seg, meta, G, SG, t, p, &ps, tot);
  if (rc != RX_OK) return rc;
  if ((rc = patch_check_meta("rx_patch_tracks_host", p, p->meta))) return rc;
  if (!t) G = SG = 0;
  for (size_t j = 0; j < ps.size(); ++j) {  // the kernel's steps (rx_cull.hip, k_patch_slots) with one lane
    const rx_patch_slot& d = ps[j];
    const int32_t k = d.slot, W = d.W;
    const double* s = p->seg + 8 * (size_t)d.src0;
    const double* w = p->wp + 2 * (size_t)d.src0;
    const double* m = p->meta + 8 * j;
    rx_cull_copy_rows<2>(w, wp + 2 * (size_t)d.wp0, W, 0, 1);
    rx_cull_copy_rows<2>(p->nrm + 2 * (size_t)d.src0, nrm + 2 * (size_t)d.wp0, W, 0, 1);
    rx_cull_copy_rows<4>(s, seg + 8 * (size_t)d.wp0, 2 * W, 0, 1);
    for (int c = 0; c < 8; ++c) meta[8 * (size_t)k + c] = m[c];
    if (!t) continue;
    rx_cull_slot o = {0, 0, 0, 0, tot[0], tot[1], t->chunk_box, t->super_box, t->wchunk_box, t->wsuper_box,
                      t->chunk_box_f, t->super_box_f};
    double b[4], longest, geo[4] = {0.0, 0.0, 0.0, 0.0};
    rx_cull_extent(s, W, 0, 1, t->seg_f + 8 * (size_t)d.wp0, b, &longest);
    if (G > 0) {
      rx_cull_geo(b, rx_cull_reach(s, W, 0, 1, 0.5 * (b[0] + b[2]), 0.5 * (b[1] + b[3])), longest, geo);
      o.chunk0 = d.chunk0;
      o.super0 = SG > 0 ? d.super0 : 0;
      o.wchunk0 = d.wchunk0;
      o.wsuper0 = d.wsuper0;
      rx_cull_boxes(s, w, W, G, SG, 0, 1, &o);
      for (int c = 0; c < 4; ++c) t->slot_geo[4 * (size_t)k + c] = geo[c];
    }
    rx_cull_header((rx_slot_hdr*)t->slot_hdr + k, d.wp0, W, &o, geo, m);
  }
  return RX_OK;
}

// ---- rendering (ABI v25, additive) ---------------------------------------------
// One body per device / host pair: the checks, then the kernel's launch or, with host, its twin's
// loops (rx_raster_host.cpp).
static int raster_static(const char* fn, bool host, int32_t n, int32_t size, int32_t n_edges, const int32_t* edge_off,
                         const int32_t* edges, uint8_t* layer, void* stream) {
  if (n <= 0 || n > RX_RASTER_MAX_IMAGES) return fail(RX_EINVAL, "%s: n=%d outside 1..%d", fn, n, RX_RASTER_MAX_IMAGES);
  if (size < RX_RASTER_SIZE_MIN || size > RX_RASTER_SIZE_MAX)
    return fail(RX_EINVAL, "%s: size=%d outside %d..%d", fn, size, RX_RASTER_SIZE_MIN, RX_RASTER_SIZE_MAX);
  if (n_edges < 0) return fail(RX_EINVAL, "%s: n_edges=%d is negative", fn, n_edges);
  if (!edge_off) return fail(RX_EINVAL, "%s: null pointer: edge_off", fn);
  if (!edges) return fail(RX_EINVAL, "%s: null pointer: edges", fn);
  if (!layer) return fail(RX_EINVAL, "%s: null pointer: layer", fn);
  if (!host) return launched(fn, rx_launch_raster_static(n, size, n_edges, edge_off, edges, layer, (hipStream_t)stream));
  rx_host_raster_static(n, size, n_edges, edge_off, edges, layer);
  return RX_OK;
}

// frame = 0: what rx_raster_trail reads; 1: what rx_raster_frame reads.
static int raster_io_args(const char* fn, const rx_raster_io* r, int frame) {
  if (!r) return fail(RX_EINVAL, "%s: null pointer: r", fn);
  if (r->size < RX_RASTER_SIZE_MIN || r->size > RX_RASTER_SIZE_MAX)
    return fail(RX_EINVAL, "%s: size=%d outside %d..%d", fn, r->size, RX_RASTER_SIZE_MIN, RX_RASTER_SIZE_MAX);
  if (r->A != 1 && r->A != 2) return fail(RX_EINVAL, "%s: A=%d must be 1 or 2", fn, r->A);
  if (r->K <= 0 || r->K > RX_RASTER_MAX_IMAGES)
    return fail(RX_EINVAL, "%s: K=%d outside 1..%d", fn, r->K, RX_RASTER_MAX_IMAGES);
  if (r->n_envs <= 0) return fail(RX_EINVAL, "%s: n_envs=%d must be > 0", fn, r->n_envs);
#define RX_RASTER_PTR(f) \
  if (!r->f) return fail(RX_EINVAL, "%s: null pointer: " #f, fn)
  RX_RASTER_PTR(env_ids);
  RX_RASTER_PTR(x);
  RX_RASTER_PTR(y);
  RX_RASTER_PTR(view);
  RX_RASTER_PTR(trail);
  if (!frame) {
    RX_RASTER_PTR(last);
    return RX_OK;
  }
  RX_RASTER_PTR(angle);
  RX_RASTER_PTR(layer_of);
  RX_RASTER_PTR(layer);
  RX_RASTER_PTR(out);
  RX_RASTER_PTR(out_off);
#undef RX_RASTER_PTR
  if (r->n_layers <= 0) return fail(RX_EINVAL, "%s: n_layers=%d must be > 0", fn, r->n_layers);
  if (r->out_pitch < 0) return fail(RX_EINVAL, "%s: out_pitch=%lld is negative", fn, (long long)r->out_pitch);
  if (r->out_pitch < 3 * (int64_t)r->size)
    return fail(RX_EINVAL, "%s: out_pitch=%lld below 3*size=%d", fn, (long long)r->out_pitch, 3 * r->size);
  if (r->out_size < 0) return fail(RX_EINVAL, "%s: out_size=%lld is negative", fn, (long long)r->out_size);
  return RX_OK;
}

static int raster_io(const char* fn, bool host, const rx_raster_io* r, int frame, void* stream) {
  const int rc = raster_io_args(fn, r, frame);
  if (rc != RX_OK) return rc;
  const hipStream_t s = (hipStream_t)stream;
  if (!host) return launched(fn, frame ? rx_launch_raster_frame(r, s) : rx_launch_raster_trail(r, s));
  frame ? rx_host_raster_frame(r) : rx_host_raster_trail(r);
  return RX_OK;
}

int rx_raster_static(int32_t n, int32_t size, int32_t n_edges, const int32_t* edge_off, const int32_t* edges,
                     uint8_t* layer, void* stream) {
  return raster_static("rx_raster_static", false, n, size, n_edges, edge_off, edges, layer, stream);
}
int rx_raster_static_host(int32_t n, int32_t size, int32_t n_edges, const int32_t* edge_off, const int32_t* edges,
                          uint8_t* layer, void* stream) {
  return raster_static("rx_raster_static_host", true, n, size, n_edges, edge_off, edges, layer, stream);
}
int rx_raster_trail(const rx_raster_io* r, void* stream) { return raster_io("rx_raster_trail", false, r, 0, stream); }
int rx_raster_trail_host(const rx_raster_io* r, void* stream) { return raster_io("rx_raster_trail_host", true, r, 0, stream); }
int rx_raster_frame(const rx_raster_io* r, void* stream) { return raster_io("rx_raster_frame", false, r, 1, stream); }
int rx_raster_frame_host(const rx_raster_io* r, void* stream) { return raster_io("rx_raster_frame_host", true, r, 1, stream); }
