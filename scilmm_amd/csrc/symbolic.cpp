// Host-side symbolic analysis: union pattern, fill-reducing ordering, elimination tree, postorder,
// column counts, (relaxed) supernodes, supernode row structures, left-looking update schedule,
// value-assembly maps.  See symbolic.h.  Replaces cholmod_analyze as reached from the reference at
// scilmm/SparseCholesky.py:22-26 / scilmm/Estimation/LMM.py:20-24, but runs once per pattern.
// (The image of an analysis on disk: symbolic_image.cpp.)
//
// All algorithms are written from their published descriptions (Liu 1990 elimination tree with
// path compression; Gilbert, Ng & Peyton 1994 skeleton column counts; Ashcraft & Grimes 1989 relaxed
// supernode amalgamation); no third-party source was available in this container.
#include "host_threads.h"
#include "symbolic.h"

#include <algorithm>
#include <atomic>
#include <cassert>
#include <cstring>
#include <numeric>
#include <queue>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <memory>
#include <thread>

namespace scilmm {

namespace {

// team size of the bucket passes that count / fill with relaxed atomics: beyond a socket's worth of cores the cache-line
// traffic of the shared counters costs more than the extra threads bring (measured on the 256-core GPU host)
#define BUCKET_THREADS std::min(16, host_threads())

// CSC-lower (strict or with diagonal) <-> CSR-lower transpose of a pattern.
void transpose_pattern(int32_t n, const std::vector<int64_t>& ptr, const std::vector<int32_t>& idx,
                       std::vector<int64_t>& tptr, std::vector<int32_t>& tidx) {
  // (count and fill with relaxed atomics on all host cores; the lists of a row come out in arbitrary order, which
  // its only reader -- Liu's elimination-tree algorithm -- does not depend on)
  tptr.assign(n + 1, 0);
  const int64_t nz = (int64_t)idx.size();
#pragma omp parallel for schedule(static) num_threads(BUCKET_THREADS)
  for (int64_t e = 0; e < nz; ++e) __atomic_fetch_add(&tptr[idx[e] + 1], 1, __ATOMIC_RELAXED);
  for (int32_t i = 0; i < n; ++i) tptr[i + 1] += tptr[i];
  tidx.resize(idx.size());
  std::vector<int64_t> fill(tptr.begin(), tptr.end() - 1);
#pragma omp parallel for schedule(dynamic, 4096) num_threads(BUCKET_THREADS)
  for (int32_t j = 0; j < n; ++j)
    for (int64_t e = ptr[j]; e < ptr[j + 1]; ++e) tidx[__atomic_fetch_add(&fill[idx[e]], 1, __ATOMIC_RELAXED)] = j;
}

// Liu's algorithm. rptr/ridx: for each row i the columns k < i with A_ik != 0.
void etree(int32_t n, const std::vector<int64_t>& rptr, const std::vector<int32_t>& ridx, std::vector<int32_t>& parent) {
  parent.assign(n, -1);
  std::vector<int32_t> anc(n, -1);
  for (int32_t i = 0; i < n; ++i) {
    for (int64_t e = rptr[i]; e < rptr[i + 1]; ++e) {
      int32_t k = ridx[e];
      while (k != -1 && k < i) {
        int32_t nx = anc[k];
        anc[k] = i;
        if (nx == -1) parent[k] = i;
        k = nx;
      }
    }
  }
}

// Postorder with children visited in increasing label order. post[k] = node visited k-th.
void postorder(int32_t n, const std::vector<int32_t>& parent, std::vector<int32_t>& post) {
  std::vector<int32_t> head(n, -1), next(n, -1);
  for (int32_t j = n - 1; j >= 0; --j) {
    if (parent[j] == -1) continue;
    next[j] = head[parent[j]];
    head[parent[j]] = j;
  }
  post.resize(n);
  int32_t k = 0;
  std::vector<int32_t> stack;
  for (int32_t r = 0; r < n; ++r) {
    if (parent[r] != -1) continue;
    stack.push_back(r);
    while (!stack.empty()) {
      int32_t p = stack.back();
      int32_t c = head[p];
      if (c == -1) {
        post[k++] = p;
        stack.pop_back();
      } else {
        head[p] = next[c];
        stack.push_back(c);
      }
    }
  }
}

int32_t find_root(std::vector<int32_t>& anc, int32_t x) {
  int32_t r = x;
  while (anc[r] != r) r = anc[r];
  while (anc[x] != r) {
    int32_t nx = anc[x];
    anc[x] = r;
    x = nx;
  }
  return r;
}

// Skeleton column counts for an arbitrary (topologically valid) labelling; post[k] = k-th node of a
// postorder of the etree.  cptr/cidx: for each column j the rows i > j with A_ij != 0.
void column_counts(int32_t n, const std::vector<int32_t>& parent, const std::vector<int32_t>& post,
                   const std::vector<int64_t>& cptr, const std::vector<int32_t>& cidx, std::vector<int32_t>& cc) {
  std::vector<int32_t> first(n, -1);
  std::vector<int64_t> delta(n);
  for (int32_t k = 0; k < n; ++k) {
    int32_t j = post[k];
    delta[j] = (first[j] == -1) ? 1 : 0;  // leaf of the etree
    for (; j != -1 && first[j] == -1; j = parent[j]) first[j] = k;
  }
  std::vector<int32_t> maxfirst(n, -1), prevleaf(n, -1), anc(n);
  std::iota(anc.begin(), anc.end(), 0);
  for (int32_t k = 0; k < n; ++k) {
    const int32_t j = post[k];
    if (parent[j] != -1) delta[parent[j]]--;
    for (int64_t e = cptr[j]; e < cptr[j + 1]; ++e) {
      int32_t i = cidx[e];
      if (i <= j) continue;
      if (first[j] <= maxfirst[i]) continue;  // j is not a leaf of row subtree i
      maxfirst[i] = first[j];
      int32_t jprev = prevleaf[i];
      prevleaf[i] = j;
      delta[j]++;
      if (jprev != -1) {
        int32_t q = find_root(anc, jprev);
        delta[q]--;
      }
    }
    if (parent[j] != -1) anc[j] = parent[j];
  }
  cc.resize(n);
  for (int32_t k = 0; k < n; ++k) {
    const int32_t j = post[k];
    cc[j] = (int32_t)delta[j];
    if (parent[j] != -1) delta[parent[j]] += delta[j];
  }
}

}  // namespace

// Fill statistics of the Cholesky factor of a symmetric pattern under a given permutation (perm[new] = old):
// elimination tree + skeleton column counts only (no supernodes, no schedules).  Used by the ordering study and by
// the nested-dissection code to compare candidate orderings.
void fill_count(int32_t n, const int64_t* g_ptr, const int32_t* g_idx, const int32_t* perm, int64_t* nnzL, double* flops,
                int32_t* max_cc, int32_t* colcount_out) {
  std::vector<int32_t> iperm(n);
  for (int32_t i = 0; i < n; ++i) iperm[perm ? perm[i] : i] = i;
  std::vector<int64_t> cptr(n + 1, 0), rptr;
  std::vector<int32_t> cidx, ridx;
  for (int32_t i = 0; i < n; ++i)
    for (int64_t e = g_ptr[i]; e < g_ptr[i + 1]; ++e) {
      const int32_t j = g_idx[e];
      if (j < 0 || j >= n || j >= i) continue;  // each undirected edge once (from its larger endpoint)
      cptr[std::min(iperm[i], iperm[j]) + 1]++;
    }
  for (int32_t i = 0; i < n; ++i) cptr[i + 1] += cptr[i];
  cidx.resize(cptr[n]);
  {
    std::vector<int64_t> fill(cptr.begin(), cptr.end() - 1);
    for (int32_t i = 0; i < n; ++i)
      for (int64_t e = g_ptr[i]; e < g_ptr[i + 1]; ++e) {
        const int32_t j = g_idx[e];
        if (j < 0 || j >= n || j >= i) continue;
        const int32_t a = iperm[i], b = iperm[j];
        cidx[fill[std::min(a, b)]++] = std::max(a, b);
      }
  }
  transpose_pattern(n, cptr, cidx, rptr, ridx);
  std::vector<int32_t> parent, post, cc;
  etree(n, rptr, ridx, parent);
  postorder(n, parent, post);
  column_counts(n, parent, post, cptr, cidx, cc);
  int64_t nz = 0;
  double fl = 0;
  int32_t mx = 0;
  for (int32_t j = 0; j < n; ++j) {
    nz += cc[j];
    fl += (double)cc[j] * (double)cc[j];
    mx = std::max(mx, cc[j]);
  }
  if (nnzL) *nnzL = nz;
  if (flops) *flops = fl;
  if (max_cc) *max_cc = mx;
  if (colcount_out) std::memcpy(colcount_out, cc.data(), sizeof(int32_t) * (size_t)n);
}

// ------------------------------------------------------------------------------------------------
// The analysis: symbolic_analyze (at the end of this section) is the list of its stages.

AnalysisSwitches read_analysis_switches() {
  AnalysisSwitches sw;
  const char* gate = getenv("SCILMM_TUNING");
  if (gate && gate[0] == '1') {
    if (const char* e = getenv("SCILMM_TAIL_ELIG")) sw.tail_elig = atof(e);
    if (const char* e = getenv("SCILMM_TAIL_DELAY")) sw.tail_delay = atoi(e);
    if (const char* e = getenv("SCILMM_TAIL_WIDE")) sw.tail_wide = atof(e);
  }
  sw.verbose = getenv("SCILMM_VERBOSE") != nullptr;
  sw.tail_dump = getenv("SCILMM_TAIL_DUMP");
  return sw;
}

namespace {

// (the order-independent hash sums that verify structural symmetry add this over the entries)
inline uint64_t mix64(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// Elimination tree of the permuted matrix straight from G.
// Liu's algorithm walks the rows of the permuted matrix in order; row i' is vertex perm[i'] and its entries left of
// the diagonal are the neighbours with a smaller new label -- no permuted copy of the pattern is needed for it.
// The neighbour lists are filtered (smaller new label only) and relabelled on all cores, a block of rows at a time;
// the sequential part reads the result as a stream.  nlarger[v] = neighbours with a larger label: the size of v's
// column in the permuted pattern (unchanged by a postorder -- adjacent vertices are ancestor and descendant).
void etree_from_g(int32_t n, const std::vector<int64_t>& gptr, const std::vector<int32_t>& gidx, const std::vector<int32_t>& perm,
                  const std::vector<int32_t>& iperm, std::vector<int32_t>& parent, std::vector<int32_t>& nlarger) {
  parent.assign(n, -1);
  nlarger.assign(n, 0);
  std::vector<int32_t> anc(n, -1);
  constexpr int32_t BLK = 32768;
  const int32_t nblk = (n + BLK - 1) / BLK;
  std::vector<int32_t> buf[2], bcnt[2];
  std::vector<int64_t> boff[2];
  for (int h = 0; h < 2; ++h) { bcnt[h].resize(BLK); boff[h].resize(BLK + 1); }
  auto filter_row = [&](int h, int32_t i0, int32_t i) {
    const int32_t v = perm[i];
    int32_t* o = buf[h].data() + boff[h][i - i0];
    int32_t m = 0;
    for (int64_t e = gptr[v]; e < gptr[v + 1]; ++e) {
      const int32_t k = iperm[gidx[e]];
      if (k < i) o[m++] = k;
    }
    bcnt[h][i - i0] = m;
    nlarger[v] = (int32_t)(gptr[v + 1] - gptr[v]) - m;
  };
  auto consume = [&](int h, int32_t i0, int32_t i1) {
    for (int32_t i = i0; i < i1; ++i) {
      const int32_t* o = buf[h].data() + boff[h][i - i0];
      for (int32_t t = 0; t < bcnt[h][i - i0]; ++t) {
        int32_t k = o[t];
        while (k != -1 && k < i) {
          const int32_t nx = anc[k];
          anc[k] = i;
          if (nx == -1) parent[k] = i;
          k = nx;
        }
      }
    }
  };
  // block b is consumed by one thread while the others filter block b + 1
  for (int32_t b = -1; b < nblk; ++b) {
    const int hn = (b + 1) & 1;
    const int32_t n0 = (b + 1) * BLK, n1 = std::min<int64_t>(n, (int64_t)(b + 2) * BLK);
    if (b + 1 < nblk) {
      boff[hn][0] = 0;
      for (int32_t i = n0; i < n1; ++i) boff[hn][i - n0 + 1] = boff[hn][i - n0] + (gptr[perm[i] + 1] - gptr[perm[i]]);
      if ((int64_t)buf[hn].size() < boff[hn][n1 - n0]) buf[hn].resize(boff[hn][n1 - n0]);
    }
    std::atomic<int32_t> next{n0};
    bool consumed = false;
#pragma omp parallel
    {
#ifdef _OPENMP
      const bool consumer = omp_get_thread_num() == 0 && omp_get_num_threads() > 1;
#else
      const bool consumer = false;
#endif
      if (consumer) {
        if (b >= 0) consume(b & 1, b * BLK, std::min<int64_t>(n, (int64_t)(b + 1) * BLK));
        consumed = true;
      } else if (b + 1 < nblk) {
        for (;;) {
          const int32_t i = next.fetch_add(64, std::memory_order_relaxed);
          if (i >= n1) break;
          for (int32_t q = i; q < std::min(n1, i + 64); ++q) filter_row(hn, n0, q);
        }
      }
    }
    if (!consumed && b >= 0) consume(b & 1, b * BLK, std::min<int64_t>(n, (int64_t)(b + 1) * BLK));  // team of one
  }
}

// The true column counts (nnz(L), flops) of the FINAL order, taken again when the dense tail was moved: elimination tree
// + postorder + skeleton counts.  Nothing in the analysis reads them (they are reported numbers), so the recount runs
// BESIDE the rest of the analysis on a quarter of the host threads: 0.4 of the 1.7 s analysis of the 100k config, 2 of
// 20 s at 1M.  The worker reads G, perm, iperm and the permuted pattern of the Analysis that owns it -- none of them is
// modified or released once it runs: every stage after the start takes the Analysis const -- and writes a vector of
// its own, which join() hands over.  The destructor joins, so that no way out of symbolic_analyze, an exception
// included, leaves the worker behind or destroys a joinable thread.
class Recount {
 public:
  ~Recount() {
    if (worker.joinable()) worker.join();
  }
  bool running() const { return worker.joinable(); }
  void start(int32_t n, const std::vector<int64_t>& gptr, const std::vector<int32_t>& gidx, const std::vector<int32_t>& perm,
             const std::vector<int32_t>& iperm, const std::vector<int64_t>& cptr, const std::vector<int32_t>& cidx) {
    worker = std::thread([this, n, &gptr, &gidx, &perm, &iperm, &cptr, &cidx]() {
      try {
#ifdef _OPENMP
        omp_set_num_threads(std::max(1, host_threads() / 4));
#endif
        std::vector<int32_t> tpar, tnl, tpost;
        etree_from_g(n, gptr, gidx, perm, iperm, tpar, tnl);
        postorder(n, tpar, tpost);
        column_counts(n, tpar, tpost, cptr, cidx, cc);
      } catch (...) {
        failed = std::current_exception();  // rethrown by join() on the main thread
      }
    });
  }
  std::vector<int32_t> join() {
    worker.join();
    if (failed) std::rethrow_exception(failed);
    return std::move(cc);
  }

 private:
  std::thread worker;
  std::vector<int32_t> cc;
  std::exception_ptr failed;
};

struct SN { int32_t start, end, m; int64_t zeros; };  // supernode: columns [start, end), m rows, relaxation zeros so far

// Between the stages of symbolic_analyze: the inputs of one call and what a stage leaves for a later one and is not part
// of the result.  Everything a single stage needs stays a local of that stage.
struct Analysis {
  const int32_t n, K;
  const int64_t* const* const indptr;
  const int32_t* const* const indices;
  const int32_t* const perm_in;
  const SymbolicOptions opts;  // (dense_relax_wide: SCILMM_TAIL_WIDE already applied)
  const AnalysisSwitches sw;
  Symbolic& S;
  std::chrono::steady_clock::time_point lap_start = std::chrono::steady_clock::now();
  void lap(const char* what) {
    auto now = std::chrono::steady_clock::now();
    if (sw.verbose) fprintf(stderr, "[scilmm symbolic] %-28s %8.3f s\n", what, std::chrono::duration<double>(now - lap_start).count());
    lap_start = now;
  }
  // build_adjacency -> every stage that reads the pattern.  G = the union pattern without its diagonal, both halves, lists
  // ascending: the ordering, the elimination tree and the permuted pattern read it by vertex, with no scatter pass of their own.
  std::vector<int64_t> gptr;
  std::vector<int32_t> gidx;
  // order_vertices, etree_and_postorder (postorder composed), move_tail_to_end (tail relabelled): final from there on
  std::vector<int32_t> perm, iperm;
  std::vector<int32_t> parent, post;  // column etree and its postorder under perm
  std::vector<int32_t> nlarger;       // per VERTEX: neighbours with a larger label under perm
  // permuted_pattern: strict lower pattern by column under perm, rows ascending
  std::vector<int64_t> cptr;
  std::vector<int32_t> cidx;
  std::vector<int32_t> cc;            // count_columns; replaced by the recount's at the join
  // find_supernodes (relabelled by move_tail_to_end)
  std::vector<SN> out;
  std::vector<int32_t> snode_of;      // front of every column
  int32_t best = 0;                   // select_dense_tail: first front of the tail-to-be (nsuper: none)
  Recount recount;                    // (last member: joined before anything it reads is destroyed)
};

// The rows of front d below its own columns, cut into the runs that fall into the columns of ONE later front s (each run
// is one update pair of the left-looking schedule): fn(s, t, t2) for rows [t, t2) of sn_rows, runs in ascending order.
template <class F>
void for_each_target_run(const Analysis& a, int32_t d, F fn) {
  const Symbolic& S = a.S;
  const int64_t re = S.sn_rowptr[d + 1];
  int64_t t = S.sn_rowptr[d] + (a.out[d].end - a.out[d].start);
  while (t < re) {
    const int32_t s = a.snode_of[S.sn_rows[t]];
    int64_t t2 = t;
    while (t2 < re && a.snode_of[S.sn_rows[t2]] == s) ++t2;
    fn(s, t, t2);
    t = t2;
  }
}
// flops of the update that a run of nq rows of a front of width w, with `below` rows after the run, sends to its target
inline double run_flops(int32_t w, int64_t nq, int64_t below) {
  return (double)w * ((double)nq * ((double)nq + 1.0) + 2.0 * (double)nq * (double)below);
}

// ---------------------------------------------------------------- 1. symmetric adjacency of the union pattern
void detect_diagonal_inputs(Analysis& a) {
  a.S.is_diag.assign(a.K, 1);
  for (int32_t k = 0; k < a.K; ++k) {
    bool diag = true;
    for (int32_t i = 0; i < a.n && diag; ++i)
      for (int64_t e = a.indptr[k][i]; e < a.indptr[k][i + 1]; ++e)
        if (a.indices[k][e] != i) { diag = false; break; }
    a.S.is_diag[k] = diag ? 1 : 0;
  }
}

// Fast path, inputs stored with both halves (what SciPy hands over): row i of G is the merged row i of the inputs,
// one pass over the rows on all cores.  Structural symmetry is verified by comparing an order-independent 64-bit
// hash sum of the lower entries (i, j) with that of the mirrored upper entries; false (G untouched): the inputs store
// one half only, or are unsymmetric, and take the scatter path below, which reads the lower half alone.
bool adjacency_from_rows(Analysis& a) {
  const int32_t n = a.n, K = a.K;
  const int64_t* const* indptr = a.indptr;
  const int32_t* const* indices = a.indices;
  std::vector<int64_t> ub(n + 1, 0);
  for (int32_t i = 0; i < n; ++i) {
    int64_t len = 0;
    for (int32_t k = 0; k < K; ++k) len += indptr[k][i + 1] - indptr[k][i];
    ub[i + 1] = ub[i] + len;
  }
  std::vector<int32_t> stage(ub[n]);
  std::vector<int32_t> cnt(n), low(n);
  uint64_t hlo = 0, hup = 0;
#pragma omp parallel for schedule(dynamic, 1024) reduction(+ : hlo, hup)
  for (int32_t i = 0; i < n; ++i) {
    int32_t* r = stage.data() + ub[i];
    int64_t m = 0;
    for (int32_t k = 0; k < K; ++k)
      for (int64_t e = indptr[k][i]; e < indptr[k][i + 1]; ++e) {
        const int32_t j = indices[k][e];
        if (j >= 0 && j < n && j != i) r[m++] = j;
      }
    bool sorted = true;
    for (int64_t t = 1; t < m; ++t)
      if (r[t - 1] >= r[t]) { sorted = false; break; }
    if (!sorted) {
      std::sort(r, r + m);
      m = std::unique(r, r + m) - r;
    }
    int32_t lo = 0;
    for (int64_t t = 0; t < m; ++t) {
      const uint32_t j = (uint32_t)r[t];
      if (r[t] < i) { hlo += mix64(((uint64_t)(uint32_t)i << 32) | j); ++lo; }
      else hup += mix64(((uint64_t)j << 32) | (uint32_t)i);
    }
    cnt[i] = (int32_t)m;
    low[i] = lo;
  }
  int64_t nlow = 0, nall = 0;
  for (int32_t i = 0; i < n; ++i) { nlow += low[i]; nall += cnt[i]; }
  if (hlo != hup || nall != 2 * nlow) return false;
  for (int32_t i = 0; i < n; ++i) a.gptr[i + 1] = a.gptr[i] + cnt[i];
  a.gidx.resize(a.gptr[n]);
#pragma omp parallel for schedule(dynamic, 4096)
  for (int32_t i = 0; i < n; ++i) std::copy(stage.data() + ub[i], stage.data() + ub[i] + cnt[i], a.gidx.begin() + a.gptr[i]);
  a.S.nnz_pattern = nlow + n;
  return true;
}

// row i of the union pattern's lower half, diagonal included: ascending, without duplicates
void merged_lower_row(const Analysis& a, int32_t i, std::vector<int32_t>& row) {
  row.assign(1, i);
  for (int32_t k = 0; k < a.K; ++k)
    for (int64_t e = a.indptr[k][i]; e < a.indptr[k][i + 1]; ++e) {
      const int32_t j = a.indices[k][e];
      if (j < 0 || j >= a.n) continue;
      if (j <= i) row.push_back(j);
    }
  std::sort(row.begin(), row.end());
  row.erase(std::unique(row.begin(), row.end()), row.end());
}

// Scatter path: the merged lower half U first (counted, then filled), G from it on all cores: the lower half of a vertex
// is its own row; the upper half is counted and filled with relaxed atomics and then sorted, so the result does not
// depend on the thread schedule.
void adjacency_from_lower_half(Analysis& a) {
  const int32_t n = a.n;
  std::vector<int64_t>& gptr = a.gptr;
  std::vector<int32_t>& gidx = a.gidx;
  std::vector<int64_t> uptr(n + 1, 0);
  std::vector<int32_t> uidx;
  {
    std::vector<int64_t> cnt(n, 0);
#pragma omp parallel for schedule(dynamic, 1024)
    for (int32_t i = 0; i < n; ++i) {
      std::vector<int32_t> tmp;
      merged_lower_row(a, i, tmp);
      cnt[i] = (int64_t)tmp.size();
    }
    for (int32_t i = 0; i < n; ++i) uptr[i + 1] = uptr[i] + cnt[i];
    uidx.resize(uptr[n]);
#pragma omp parallel for schedule(dynamic, 1024)
    for (int32_t i = 0; i < n; ++i) {
      std::vector<int32_t> tmp;
      merged_lower_row(a, i, tmp);
      std::copy(tmp.begin(), tmp.end(), uidx.begin() + uptr[i]);
    }
  }
  a.S.nnz_pattern = uptr[n];
  std::vector<int64_t> up(n, 0);
#pragma omp parallel for schedule(dynamic, 4096) num_threads(BUCKET_THREADS)
  for (int32_t i = 0; i < n; ++i)
    for (int64_t e = uptr[i]; e < uptr[i + 1]; ++e) {
      const int32_t j = uidx[e];
      if (j != i) __atomic_fetch_add(&up[j], 1, __ATOMIC_RELAXED);
    }
  for (int32_t i = 0; i < n; ++i) gptr[i + 1] = gptr[i] + (uptr[i + 1] - uptr[i] - 1) + up[i];
  gidx.resize(gptr[n]);
  std::vector<int64_t> fill(n);
#pragma omp parallel for schedule(dynamic, 4096)
  for (int32_t i = 0; i < n; ++i) {
    int64_t f = gptr[i];
    for (int64_t e = uptr[i]; e < uptr[i + 1]; ++e)
      if (uidx[e] != i) gidx[f++] = uidx[e];
    fill[i] = f;
  }
#pragma omp parallel for schedule(dynamic, 4096) num_threads(BUCKET_THREADS)
  for (int32_t i = 0; i < n; ++i)
    for (int64_t e = uptr[i]; e < uptr[i + 1]; ++e) {
      const int32_t j = uidx[e];
      if (j != i) gidx[__atomic_fetch_add(&fill[j], 1, __ATOMIC_RELAXED)] = i;
    }
#pragma omp parallel for schedule(dynamic, 1024)
  for (int32_t i = 0; i < n; ++i) std::sort(gidx.begin() + (gptr[i + 1] - up[i]), gidx.begin() + gptr[i + 1]);
}

void build_adjacency(Analysis& a) {
  a.gptr.assign((size_t)a.n + 1, 0);
  const bool have_g = adjacency_from_rows(a);
  if (a.sw.verbose) fprintf(stderr, "[scilmm symbolic] inputs %s\n", have_g ? "store both halves: adjacency read row by row" : "do not store both halves symmetrically: lower half scattered");
  if (!have_g) adjacency_from_lower_half(a);
}

// ---------------------------------------------------------------- 2. ordering
// false: the user's permutation is refused, S.error says why
bool order_vertices(Analysis& a) {
  const int32_t n = a.n;
  const SymbolicOptions& opts = a.opts;
  std::vector<int32_t>& perm = a.perm;
  perm.resize(n);
  if (opts.ordering == 2) {
    if (!a.perm_in) { a.S.error = "user ordering requested but no permutation given"; return false; }
    std::vector<uint8_t> seen(n, 0);
    for (int32_t i = 0; i < n; ++i) {
      int32_t p = a.perm_in[i];
      if (p < 0 || p >= n || seen[p]) { a.S.error = "invalid user permutation"; return false; }
      seen[p] = 1;
      perm[i] = p;
    }
  } else if (opts.ordering == 1) {
    std::iota(perm.begin(), perm.end(), 0);
  } else if (opts.ordering == 3 || opts.ordering == 4) {
    NdOptions ndo;
    ndo.oksep = opts.nd_oksep;
    NdStats nds;
    nd_order(n, a.gptr.data(), a.gidx.data(), perm.data(), ndo, &nds);
    if (a.sw.verbose)
      fprintf(stderr, "[scilmm symbolic] nested dissection: %d -> %d compressed vertices, %lld separators, largest %lld\n", n,
              nds.n_compressed, (long long)nds.n_separators, (long long)nds.top_separator);
    if (opts.ordering == 4) {
      // keep whichever ordering gives fewer factor flops (elimination tree + column counts only: cheap)
      std::vector<int32_t> p2(n);
      amd_order(n, a.gptr.data(), a.gidx.data(), p2.data(), opts.amd_dense);
      double f_nd = 0, f_amd = 0;
      fill_count(n, a.gptr.data(), a.gidx.data(), perm.data(), nullptr, &f_nd, nullptr, nullptr);
      fill_count(n, a.gptr.data(), a.gidx.data(), p2.data(), nullptr, &f_amd, nullptr, nullptr);
      if (a.sw.verbose) fprintf(stderr, "[scilmm symbolic] factor flops: nested dissection %.4g, minimum degree %.4g\n", f_nd, f_amd);
      if (f_amd < f_nd) perm.swap(p2);
    }
  } else {
    amd_order(n, a.gptr.data(), a.gidx.data(), perm.data(), opts.amd_dense);
  }
  a.iperm.resize(n);
  for (int32_t i = 0; i < n; ++i) a.iperm[perm[i]] = i;
  return true;
}

// ---------------------------------------------------------------- 3. etree + postorder straight from G
void etree_and_postorder(Analysis& a) {
  const int32_t n = a.n;
  std::vector<int32_t>&perm = a.perm, &iperm = a.iperm, &parent = a.parent, &post = a.post;
  etree_from_g(n, a.gptr, a.gidx, perm, iperm, parent, a.nlarger);
  postorder(n, parent, post);
  // A user-supplied permutation is honoured exactly (parity with an oracle factor of the same P);
  // otherwise the ordering is composed with the etree postorder (same fill, contiguous supernodes).
  if (a.opts.ordering != 2) {
    std::vector<int32_t> perm2(n), pinv(n);
    for (int32_t k = 0; k < n; ++k) {
      perm2[k] = perm[post[k]];
      pinv[post[k]] = k;
    }
    std::vector<int32_t> par2(n);
    for (int32_t j = 0; j < n; ++j) par2[pinv[j]] = parent[j] == -1 ? -1 : pinv[parent[j]];
    parent.swap(par2);
    perm.swap(perm2);
    for (int32_t i = 0; i < n; ++i) iperm[perm[i]] = i;
    std::iota(post.begin(), post.end(), 0);
  }
}

// ---------------------------------------------------------------- 4. permuted strict-lower pattern by column
// column c = vertex perm[c]; its rows are the neighbours with a larger new label (nlarger[perm[c]] of them), sorted
// (column by column, straight from G, no scatter)
void permuted_pattern(Analysis& a) {
  const int32_t n = a.n;
  std::vector<int64_t>& cptr = a.cptr;
  std::vector<int32_t>& cidx = a.cidx;
  cptr.assign((size_t)n + 1, 0);
  for (int32_t c = 0; c < n; ++c) cptr[c + 1] = cptr[c] + a.nlarger[a.perm[c]];
  cidx.resize(cptr[n]);
#pragma omp parallel for schedule(dynamic, 1024)
  for (int32_t c = 0; c < n; ++c) {
    const int32_t v = a.perm[c];
    int64_t f = cptr[c];
    for (int64_t e = a.gptr[v]; e < a.gptr[v + 1]; ++e) {
      const int32_t r = a.iperm[a.gidx[e]];
      if (r > c) cidx[f++] = r;
    }
    std::sort(cidx.begin() + cptr[c], cidx.begin() + cptr[c + 1]);
  }
}

// ---------------------------------------------------------------- 5. column counts
void report_column_counts(const std::vector<int32_t>& cc, Symbolic& S) {
  S.nnzL = 0;
  S.flops = 0;
  for (int32_t c : cc) {
    S.nnzL += c;
    S.flops += (double)c * (double)c;
  }
}

void count_columns(Analysis& a) {
  column_counts(a.n, a.parent, a.post, a.cptr, a.cidx, a.cc);
  report_column_counts(a.cc, a.S);
}

// ---------------------------------------------------------------- 6. supernodes (fundamental, then relaxed)
void find_supernodes(Analysis& a) {
  const int32_t n = a.n;
  const SymbolicOptions& opts = a.opts;
  const std::vector<int32_t>&parent = a.parent, &cc = a.cc;
  std::vector<SN>& out = a.out;
  {
    int32_t j = 0;
    std::vector<int32_t> nchild(n, 0);
    for (int32_t c = 0; c < n; ++c)
      if (parent[c] != -1) nchild[parent[c]]++;
    while (j < n) {
      int32_t s = j;
      while (j + 1 < n && parent[j] == j + 1 && cc[j + 1] == cc[j] - 1 && nchild[j + 1] == 1) ++j;
      ++j;
      SN p{s, j, cc[s], 0};
      // relaxed amalgamation with the immediately preceding supernode while it is a child
      while (!out.empty()) {
        SN& c = out.back();
        int32_t pc = parent[c.end - 1];
        if (pc < p.start || pc >= p.end) break;
        int64_t wc = c.end - c.start, wp = p.end - p.start;
        int64_t mnew = wc + p.m;
        int64_t wnew = wc + wp;
        int64_t z = c.zeros + p.zeros + wc * (wc + p.m - c.m);
        double tot = (double)wnew * (double)mnew - (double)wnew * (double)(wnew - 1) / 2.0;
        double frac = (double)z / tot;
        bool merge = (wnew <= opts.relax_small) || (wnew <= opts.relax_w1 && frac < opts.relax_z1) ||
                     (wnew <= opts.relax_w2 && frac < opts.relax_z2) || (frac < opts.relax_z3);
        // no width cap here: a chain that merges without (much) fill is merged whole and then cut into blocks of
        // exactly max_width columns below, so that the update kernel's 128x128 tiles are full in dense regions
        if (!merge) break;
        p.start = c.start;
        p.m = (int32_t)mnew;
        p.zeros = z;
        out.pop_back();
      }
      out.push_back(p);
    }
  }
  // optional splitting of very wide supernodes (keeps kernels' LDS tiles bounded)
  if (opts.max_width > 0) {
    std::vector<SN> sp;
    for (auto& s : out) {
      int32_t w = s.end - s.start;
      if (w <= opts.max_width) { sp.push_back(s); continue; }
      for (int32_t st = s.start; st < s.end; st += opts.max_width) {
        const int32_t ww = std::min<int32_t>(opts.max_width, s.end - st);
        sp.push_back(SN{st, st + ww, s.m - (st - s.start), 0});
      }
    }
    out.swap(sp);
  }
  const int32_t ns = (int32_t)out.size();
  a.S.nsuper = ns;
  a.S.sn_start.resize(ns + 1);
  for (int32_t s = 0; s < ns; ++s) a.S.sn_start[s] = out[s].start;
  a.S.sn_start[ns] = n;
  a.snode_of.resize(n);
  for (int32_t s = 0; s < ns; ++s)
    for (int32_t j = out[s].start; j < out[s].end; ++j) a.snode_of[j] = s;
}

// ---------------------------------------------------------------- 7. row structure of every supernode
void front_row_structures(Analysis& a) {
  const int32_t n = a.n, ns = a.S.nsuper;
  Symbolic& S = a.S;
  const std::vector<SN>& out = a.out;
  const std::vector<int64_t>& cptr = a.cptr;
  const std::vector<int32_t>& cidx = a.cidx;
  S.sn_rowptr.assign(ns + 1, 0);
  S.sn_parent.assign(ns, -1);
  // rows contributed by the input pattern itself (the columns of A inside the front), on all cores; what is left
  // for the sequential sweep below is the merge of the children's row lists (a child always precedes its parent)
  std::vector<std::vector<int32_t>> arows(ns);
#pragma omp parallel
  {
    std::vector<int32_t> mk(n, -1);
#pragma omp for schedule(dynamic, 64)
    for (int32_t s = 0; s < ns; ++s) {
      const int32_t c0 = out[s].start, c1 = out[s].end;
      std::vector<int32_t>& ar = arows[s];
      for (int32_t j = c0; j < c1; ++j)
        for (int64_t e = cptr[j]; e < cptr[j + 1]; ++e) {
          const int32_t i = cidx[e];
          if (i >= c1 && mk[i] != s) { mk[i] = s; ar.push_back(i); }
        }
    }
  }
  std::vector<int32_t> chead(ns, -1), cnext(ns, -1);
  std::vector<int32_t> mark(n, -1);
  std::vector<int32_t> tmp;
  S.sn_rows.reserve((size_t)(S.nnzL / 4 + n));
  for (int32_t s = 0; s < ns; ++s) {
    int32_t c0 = out[s].start, c1 = out[s].end;
    tmp.swap(arows[s]);
    std::vector<int32_t>().swap(arows[s]);
    for (int32_t i : tmp) mark[i] = s;
    for (int32_t c = chead[s]; c != -1; c = cnext[c]) {
      int64_t b = S.sn_rowptr[c], e2 = S.sn_rowptr[c + 1];
      int32_t wc = out[c].end - out[c].start;
      for (int64_t e = b + wc; e < e2; ++e) {
        int32_t i = S.sn_rows[e];
        if (i >= c1 && mark[i] != s) { mark[i] = s; tmp.push_back(i); }
      }
    }
    for (int32_t j = c0; j < c1; ++j) S.sn_rows.push_back(j);
    const size_t first = S.sn_rows.size();
    if ((int64_t)tmp.size() * 16 > (int64_t)(n - c1)) {
      // long list (the fronts of the trailing clique hold most of the later columns): read it off the marks
      for (int32_t i = c1; i < n; ++i)
        if (mark[i] == s) S.sn_rows.push_back(i);
    } else {
      std::sort(tmp.begin(), tmp.end());
      S.sn_rows.insert(S.sn_rows.end(), tmp.begin(), tmp.end());
    }
    S.sn_rowptr[s + 1] = (int64_t)S.sn_rows.size();
    if (!tmp.empty()) {
      int32_t p = a.snode_of[S.sn_rows[first]];
      S.sn_parent[s] = p;
      cnext[s] = chead[p];
      chead[p] = s;
    }
    tmp.clear();
  }
}

// ---------------------------------------------------------------- 7a. dense tail: which fronts
// The top of a pedigree factor (16.6k columns at the 100k config, 170k at 1M; > 75 % / > 99 % of the flops) consists
// of fronts whose row lists are "almost every later column".  Padding those lists to EVERY later column (explicit
// zeros, like relaxed amalgamation) turns that part into one dense lower-triangular matrix cut into block columns:
// updates inside it need no index lists, no descriptors and no gather.
// The tail T is an ancestor-closed set of fronts, grown from the roots of the supernodal tree downwards: among the
// fronts whose parent is already in T the one with the longest true row list is taken next, as long as its own list
// fills at least half of its padded one and the padded flop count of the whole tail stays within dense_relax of the
// true one.  T need not be a chain of the tree: at the 1M config two chains of near-dense fronts (45 x 128 columns
// with 126k rows each beside the main one) merge 46 levels above the tail's start; as a side branch their updates
// of the tail went through the gather path at 11 TFLOP/s (a fifth of the factorization time), inside T they are
// k_dense work.  The fronts of T are moved to the end of the elimination order (children still precede parents, so
// the fill is unchanged) in the reverse order in which they were taken.
// A user-supplied permutation is never changed: then T is the trailing chain (parent = next front) only.
void select_tail_chain(Analysis& a) {
  const Symbolic& S = a.S;
  const int32_t ns = S.nsuper;
  double fl_dense = 0.0, fl_true = 0.0;
  for (int32_t q = ns - 1; q >= 0; --q) {
    if (q < ns - 1 && S.sn_parent[q] != q + 1) break;
    const double w = a.out[q].end - a.out[q].start, mt = (double)(S.sn_rowptr[q + 1] - S.sn_rowptr[q]), md = (double)(a.n - a.out[q].start);
    fl_dense += w * md * md;
    fl_true += w * mt * mt;
    if (fl_dense <= a.opts.dense_relax * fl_true) a.best = q;
    else if (fl_dense > 1.5 * fl_true) break;
  }
}

struct Tail {
  std::vector<int32_t> taken;        // the fronts of T in their new order: the reverse of the order in which they were taken
  int64_t cols = 0;                  // columns of T
  double ratio = 0.0;                // padded / true flops of T
  size_t ncl = 0;                    // the last ncl fronts of `taken` are (all but) a clique
  std::vector<int32_t> clique_cols;  // ncl >= 2: the clique's columns (old labels) in their new order
};

Tail grow_tail_from_roots(const Analysis& a) {
  const Symbolic& S = a.S;
  const SymbolicOptions& opts = a.opts;
  const std::vector<SN>& out = a.out;
  const int32_t ns = S.nsuper;
  std::vector<int32_t> chead(ns, -1), cnext(ns, -1);
  for (int32_t q = 0; q < ns; ++q)
    if (S.sn_parent[q] != -1) { cnext[q] = chead[S.sn_parent[q]]; chead[S.sn_parent[q]] = q; }
  std::priority_queue<std::pair<int64_t, int32_t>> heap;  // (true rows, front): longest list first, then the later front
  for (int32_t q = 0; q < ns; ++q)
    if (S.sn_parent[q] == -1) heap.push({S.sn_rowptr[q + 1] - S.sn_rowptr[q], q});
  Tail T;
  std::vector<int32_t>& taken = T.taken;
  double fl_dense = 0.0, fl_true = 0.0;
  int64_t cols_after = 0, wide_cols = 0;
  double wide_ratio = 0.0;
  size_t nbest = 0, nwide = 0;
  FilePtr tail_dump(a.sw.tail_dump ? fopen(a.sw.tail_dump, "w") : nullptr);  // diagnostic: every candidate
  if (tail_dump) fprintf(tail_dump.get(), "taken,front,w,true_rows,padded_rows,fl_dense_before,fl_true_before\n");
  while (!heap.empty()) {
    const int32_t q = heap.top().second;
    heap.pop();
    const double w = out[q].end - out[q].start, mt = (double)(S.sn_rowptr[q + 1] - S.sn_rowptr[q]), md = (double)cols_after + w;
    if (tail_dump) fprintf(tail_dump.get(), "%d,%d,%.0f,%.0f,%.0f,%.6g,%.6g\n", (int)taken.size(), q, w, mt, md, fl_dense, fl_true);
    // (0.5: padding such a front costs at most 4 x its true flops, the ratio between the dense and the gather kernel.
    // SCILMM_TUNING=1 SCILMM_TAIL_ELIG=x: at 1M 0.3 takes 27 more fronts, starts the tail 4 levels earlier -- fewer
    // fronts behind k_outside, 7 x the cells -- and is slower, 30.2 vs 29.6 s.)
    if (mt < a.sw.tail_elig * md) continue;  // its list only gets relatively shorter as T grows: never eligible again
    fl_dense += w * md * md;
    fl_true += w * mt * mt;
    taken.push_back(q);
    cols_after += (int64_t)w;
    if (fl_dense <= opts.dense_relax * fl_true) { nbest = taken.size(); T.cols = cols_after; T.ratio = fl_dense / fl_true; }
    if (fl_dense <= opts.dense_relax_wide * fl_true) { nwide = taken.size(); wide_cols = cols_after; wide_ratio = fl_dense / fl_true; }
    if (fl_dense > std::max(1.5, opts.dense_relax_wide) * fl_true) break;
    for (int32_t c = chead[q]; c != -1; c = cnext[c]) heap.push({S.sn_rowptr[c + 1] - S.sn_rowptr[c], c});
  }
  if (T.cols >= opts.dense_wide_cols && nwide > nbest) { nbest = nwide; T.cols = wide_cols; T.ratio = wide_ratio; }
  taken.resize(nbest);
  std::reverse(taken.begin(), taken.end());
  return T;
}

// The top of T is (all but) a clique: every front's list holds >= 99 % of the later columns (1200 of the 1393
// fronts at the 1M config, fill 0.997 - 1.000) and is padded to all of them anyway.  The structure of every
// column BELOW that region depends only on which columns precede it, not on the order inside the region, so the
// region's columns may be sorted freely: by the number of lower tail fronts that have them as a row.  What a lower
// front does NOT reach (12 - 50 % of the region for the fronts below it at 1M) then sits together at the region's
// start, as whole 128-column blocks that the dense update can skip (tail_blk below), instead of being spread over
// every block as padding.  (The true fill inside the region changes by a fraction of a percent with its order:
// the column counts are taken again for the final order.)
void order_tail_clique(const Analysis& a, Tail& T) {
  const Symbolic& S = a.S;
  const std::vector<SN>& out = a.out;
  const std::vector<int32_t>& taken = T.taken;
  const size_t nbest = taken.size();
  int64_t cols = 0;
  for (size_t t = nbest; t-- > 0;) {
    const int32_t q = taken[t];
    const int64_t w = out[q].end - out[q].start;
    if ((double)(S.sn_rowptr[q + 1] - S.sn_rowptr[q]) < 0.99 * (double)(cols + w)) break;
    cols += w;
    ++T.ncl;
  }
  if (T.ncl < 2) return;
  const size_t nlow = nbest - T.ncl;
  std::vector<uint8_t> in_cl(S.nsuper, 0);
  for (size_t t = nlow; t < nbest; ++t) in_cl[taken[t]] = 1;
  std::vector<int32_t> cnt(a.n, 0);
  for (size_t t = 0; t < nlow; ++t) {
    const int32_t q = taken[t];
    for (int64_t e = S.sn_rowptr[q] + (out[q].end - out[q].start); e < S.sn_rowptr[q + 1]; ++e)
      if (in_cl[a.snode_of[S.sn_rows[e]]]) cnt[S.sn_rows[e]]++;
  }
  for (size_t t = nlow; t < nbest; ++t)
    for (int32_t j = out[taken[t]].start; j < out[taken[t]].end; ++j) T.clique_cols.push_back(j);
  if (nlow > 0) std::stable_sort(T.clique_cols.begin(), T.clique_cols.end(), [&](int32_t x, int32_t y) { return cnt[x] < cnt[y]; });
}

// New front order = the others as they are, then T; new labels front by front (clique: column by column).  Unless every
// column keeps its label: the order, the row lists, the parents (of fronts and of columns) and the permuted pattern under
// the new labels, and the recount of the column counts started beside the rest of the analysis.
void move_tail_to_end(Analysis& a, const Tail& T) {
  const int32_t n = a.n, ns = a.S.nsuper;
  Symbolic& S = a.S;
  std::vector<SN>& out = a.out;
  std::vector<uint8_t> inT(ns, 0);
  for (int32_t q : T.taken) inT[q] = 1;
  std::vector<int32_t> order;
  order.reserve(ns);
  for (int32_t q = 0; q < ns; ++q)
    if (!inT[q]) order.push_back(q);
  order.insert(order.end(), T.taken.begin(), T.taken.end());
  std::vector<int32_t> newlab(n);
  std::vector<SN> out2(ns);
  const int32_t k_cl = T.ncl >= 2 ? ns - (int32_t)T.ncl : ns;  // first clique front (new index)
  {
    int32_t c = 0;
    size_t ci = 0;
    for (int32_t k = 0; k < ns; ++k) {
      const int32_t q = order[k];
      out2[k] = out[q];
      out2[k].start = c;
      const int32_t w = out[q].end - out[q].start;
      if (k >= k_cl) {
        for (int32_t t = 0; t < w; ++t) newlab[T.clique_cols[ci++]] = c++;
      } else {
        for (int32_t j = out[q].start; j < out[q].end; ++j) newlab[j] = c++;
      }
      out2[k].end = c;
    }
  }
  bool in_place = true;
  for (int32_t j = 0; j < n && in_place; ++j) in_place = newlab[j] == j;
  if (a.sw.verbose)
    fprintf(stderr, "[scilmm symbolic] dense tail: %zu fronts (%zu of them a clique), %lld columns, padded / true flops %.3f%s\n", T.taken.size(),
            T.ncl, (long long)T.cols, T.ratio, in_place ? "" : " (moved to the end of the order)");
  if (in_place) return;
  {
    std::vector<int32_t> perm2(n);
    for (int32_t j = 0; j < n; ++j) perm2[newlab[j]] = a.perm[j];
    a.perm.swap(perm2);
    for (int32_t i = 0; i < n; ++i) a.iperm[a.perm[i]] = i;
  }
  // row lists: relabel, sort, store in the new front order (a clique front: every later column)
  std::vector<int64_t> rp2(ns + 1, 0);
  for (int32_t k = 0; k < ns; ++k)
    rp2[k + 1] = rp2[k] + (k >= k_cl ? (int64_t)(n - out2[k].start) : S.sn_rowptr[order[k] + 1] - S.sn_rowptr[order[k]]);
  std::vector<int32_t> rows2(rp2[ns]);
#pragma omp parallel for schedule(dynamic, 64)
  for (int32_t k = 0; k < ns; ++k) {
    int32_t* o = rows2.data() + rp2[k];
    if (k >= k_cl) {
      for (int32_t r = out2[k].start; r < n; ++r) o[r - out2[k].start] = r;
      continue;
    }
    const int32_t q = order[k];
    const int64_t b = S.sn_rowptr[q], e = S.sn_rowptr[q + 1];
    for (int64_t t = b; t < e; ++t) o[t - b] = newlab[S.sn_rows[t]];
    std::sort(o + (out[q].end - out[q].start), o + (e - b));  // (own columns stay first and ascending)
  }
  S.sn_rows.swap(rows2);
  S.sn_rowptr.swap(rp2);
  out.swap(out2);
  for (int32_t k = 0; k < ns; ++k) {
    S.sn_start[k] = out[k].start;
    for (int32_t j = out[k].start; j < out[k].end; ++j) a.snode_of[j] = k;
  }
  // parents (of fronts and of columns) follow from the row lists
  for (int32_t k = 0; k < ns; ++k) {
    const int64_t b = S.sn_rowptr[k], e = S.sn_rowptr[k + 1];
    const int32_t w = out[k].end - out[k].start;
    S.sn_parent[k] = e - b > w ? a.snode_of[S.sn_rows[b + w]] : -1;
    for (int32_t j = out[k].start; j + 1 < out[k].end; ++j) a.parent[j] = j + 1;
    a.parent[out[k].end - 1] = e - b > w ? S.sn_rows[b + w] : -1;
  }
  // the permuted pattern under the new labels, again straight from G
#pragma omp parallel for schedule(dynamic, 1024)
  for (int32_t c = 0; c < n; ++c) {
    const int32_t v = a.perm[c];
    int32_t m = 0;
    for (int64_t e = a.gptr[v]; e < a.gptr[v + 1]; ++e) m += a.iperm[a.gidx[e]] > c;
    a.nlarger[v] = m;
  }
  permuted_pattern(a);
  a.recount.start(n, a.gptr, a.gidx, a.perm, a.iperm, a.cptr, a.cidx);
}

void select_dense_tail(Analysis& a) {
  const int32_t ns = a.S.nsuper;
  a.S.dense_first = a.best = ns;
  if (a.opts.dense_relax > 0.0 && a.opts.ordering == 2) {
    select_tail_chain(a);
  } else if (a.opts.dense_relax > 0.0) {
    Tail T = grow_tail_from_roots(a);
    if (T.taken.size() >= 4) {
      a.best = ns - (int32_t)T.taken.size();
      order_tail_clique(a, T);
      move_tail_to_end(a, T);
    }
  }
  // the order is final (and the recount may be running: the stages below take the Analysis const)
  a.S.perm = a.perm;
  a.S.iperm = a.iperm;
  a.S.parent = a.parent;
}

// ---------------------------------------------------------------- 7b. dense tail: padding
void pad_dense_tail(const Analysis& a) {
  Symbolic& S = a.S;
  const std::vector<SN>& out = a.out;
  const int32_t n = a.n, ns = S.nsuper, best = a.best;
  if (!(a.opts.dense_relax > 0.0) || ns - best < 4) return;
  // on the TRUE row lists of the fronts about to be padded: their algorithmic update flops (as in step 10) and the block
  // pattern of the true structure (which later tail fronts does a tail front reach at all; rows ascending => fronts ascending)
  double true_tail = 0.0;
  S.tail_blk_ptr.assign((size_t)(ns - best) + 1, 0);
  for (int32_t d = best; d < ns; ++d) {
    for_each_target_run(a, d, [&](int32_t s, int64_t t, int64_t t2) {
      true_tail += run_flops(out[d].end - out[d].start, t2 - t, S.sn_rowptr[d + 1] - t2);
      S.tail_blk.push_back(s - best);
    });
    S.tail_blk_ptr[(size_t)(d - best) + 1] = (int64_t)S.tail_blk.size();
  }
  S.update_flops_pad = -true_tail;  // completed in step 10: executed(tail) - true(tail)
  S.dense_flops = true_tail;
  S.dense_first = best;
  S.sn_rows.resize((size_t)S.sn_rowptr[best]);
  for (int32_t q = best; q < ns; ++q) {
    for (int32_t r = out[q].start; r < n; ++r) S.sn_rows.push_back(r);
    S.sn_rowptr[q + 1] = (int64_t)S.sn_rows.size();
    S.sn_parent[q] = q + 1 < ns ? q + 1 : -1;  // padded: the tail is a chain in index order
  }
}

// ---------------------------------------------------------------- 8. panel offsets, levels, children
void panel_offsets_levels_children(const Analysis& a) {
  Symbolic& S = a.S;
  const int32_t ns = S.nsuper;
  S.sn_loff.assign(ns + 1, 0);
  for (int32_t s = 0; s < ns; ++s) {
    int64_t m = S.sn_rowptr[s + 1] - S.sn_rowptr[s];
    int64_t w = a.out[s].end - a.out[s].start;
    int64_t sz = m * w;
    sz = (sz + 1) & ~(int64_t)1;  // keep every panel 16-byte aligned
    S.sn_loff[s + 1] = S.sn_loff[s] + sz;
  }
  S.nnzL_stored = S.sn_loff[ns];
  S.sn_level.assign(ns, 0);
  for (int32_t s = 0; s < ns; ++s) {
    int32_t p = S.sn_parent[s];
    if (p != -1) S.sn_level[p] = std::max(S.sn_level[p], S.sn_level[s] + 1);
  }
  // (SCILMM_TUNING=1 SCILMM_TAIL_DELAY=k starts the tail chain k levels later, so that more of the prelude lies below
  // it and goes through k_outside instead of the gather path: at 1M k = 24 moves 96 % of the remaining gather combos
  // there, 2.8M -> 6.5M outside items, and the factorization takes the same 29.6 s -- the two paths cost the same.)
  if (a.sw.tail_delay != 0 && S.dense_first < ns) {
    S.sn_level[S.dense_first] += a.sw.tail_delay;
    for (int32_t q = S.dense_first + 1; q < ns; ++q) S.sn_level[q] = std::max(S.sn_level[q], S.sn_level[q - 1] + 1);
  }
  S.nlevels = 0;
  for (int32_t s = 0; s < ns; ++s) S.nlevels = std::max(S.nlevels, S.sn_level[s] + 1);

  // children lists (increasing order)
  S.child_ptr.assign(ns + 1, 0);
  for (int32_t s = 0; s < ns; ++s)
    if (S.sn_parent[s] != -1) S.child_ptr[S.sn_parent[s] + 1]++;
  for (int32_t s = 0; s < ns; ++s) S.child_ptr[s + 1] += S.child_ptr[s];
  S.child_idx.resize(S.child_ptr[ns]);
  std::vector<int64_t> fill(S.child_ptr.begin(), S.child_ptr.end() - 1);
  for (int32_t s = 0; s < ns; ++s)
    if (S.sn_parent[s] != -1) S.child_idx[fill[S.sn_parent[s]]++] = s;
}

// ---------------------------------------------------------------- 9. value-assembly maps
// pattern slots are numbered in permuted CSC order with the diagonal first in each column (S.pat_colptr).
void pattern_slot_maps(const Analysis& a) {
  Symbolic& S = a.S;
  const int32_t n = a.n, ns = S.nsuper;
  const std::vector<SN>& out = a.out;
  const std::vector<int64_t>& cptr = a.cptr;
  const std::vector<int32_t>& cidx = a.cidx;
  std::vector<int64_t>& slot_ptr = S.pat_colptr;
  slot_ptr.assign((size_t)n + 1, 0);
  for (int32_t j = 0; j < n; ++j) slot_ptr[j + 1] = slot_ptr[j] + 1 + (cptr[j + 1] - cptr[j]);
  S.asm_dst.resize(slot_ptr[n]);
  S.diag_dst.resize(n);
  S.pat_row.resize(slot_ptr[n]);
  S.nnz_pattern = slot_ptr[n];
#pragma omp parallel for schedule(dynamic, 4096)
  for (int32_t j = 0; j < n; ++j) {
    int64_t sl = slot_ptr[j];
    S.pat_row[sl++] = j;
    for (int64_t e = cptr[j]; e < cptr[j + 1]; ++e) S.pat_row[sl++] = cidx[e];
  }
  S.inv_off.assign(ns + 1, 0);
  for (int32_t s = 0; s < ns; ++s) {
    int64_t w = out[s].end - out[s].start;
    S.inv_off[s + 1] = S.inv_off[s] + ((w * w + 1) & ~(int64_t)1);
  }
#pragma omp parallel
  {
    std::vector<int32_t> pos(n, -1);
#pragma omp for schedule(dynamic, 16)
    for (int32_t s = 0; s < ns; ++s) {
      int64_t rb = S.sn_rowptr[s], re = S.sn_rowptr[s + 1];
      int64_t m = re - rb;
      const bool tail = s >= S.dense_first;  // rows = every column from the front's first on
      const int32_t c0 = out[s].start;
      if (!tail)
        for (int64_t t = rb; t < re; ++t) pos[S.sn_rows[t]] = (int32_t)(t - rb);
      for (int32_t j = c0; j < out[s].end; ++j) {
        int64_t colbase = S.sn_loff[s] + (int64_t)(j - c0) * m;
        int64_t sl = slot_ptr[j];
        S.asm_dst[sl] = colbase + (j - c0);
        S.diag_dst[j] = S.asm_dst[sl];
        ++sl;
        if (tail)
          for (int64_t e = cptr[j]; e < cptr[j + 1]; ++e) S.asm_dst[sl++] = colbase + (cidx[e] - c0);
        else
          for (int64_t e = cptr[j]; e < cptr[j + 1]; ++e) S.asm_dst[sl++] = colbase + pos[cidx[e]];
      }
    }
  }
}

// per input matrix: where does each stored lower entry go
void value_map_diagonal(const Analysis& a, int32_t k) {
  for (int32_t i = 0; i < a.n; ++i)
    for (int64_t e = a.indptr[k][i]; e < a.indptr[k][i + 1]; ++e) {
      a.S.val_slot[k].push_back(a.iperm[i]);
      a.S.val_src[k].push_back(e);
    }
}

// Fast path -- matrix k stores both halves, rows strictly ascending (canonical CSR); false: it does not, nothing written.
// Vertex v's pattern column c = new(v) is walked once: positions of its rows go to a thread-local table, and every entry
// (v, u) of row v with new(u) >= c finds its slot there -- the column is warm, nothing is searched.  The value is read
// from the stored LOWER entry: (v, u) itself if u <= v, else its mirror (u, v), whose index inside row u is the number of
// smaller columns in that row = the running count of mirrors seen while the rows are swept in ascending order
// (done per range of target rows, one range per thread, so the counts need no atomics).
bool value_map_canonical(const Analysis& a, int32_t k) {
  Symbolic& S = a.S;
  const int32_t n = a.n;
  const int64_t* ip = a.indptr[k];
  const int32_t* ix = a.indices[k];
  const std::vector<int32_t>& iperm = a.iperm;
  {
    uint64_t hlo = 0, hup = 0;
    int64_t bad = 0;
#pragma omp parallel for schedule(dynamic, 1024) reduction(+ : hlo, hup, bad)
    for (int32_t i = 0; i < n; ++i)
      for (int64_t e = ip[i]; e < ip[i + 1]; ++e) {
        const int32_t j = ix[e];
        if (j < 0 || j >= n || (e > ip[i] && ix[e - 1] >= j)) { ++bad; continue; }
        if (j < i) hlo += mix64(((uint64_t)(uint32_t)i << 32) | (uint32_t)j);
        else if (j > i) hup += mix64(((uint64_t)(uint32_t)j << 32) | (uint32_t)i);
      }
    if (bad != 0 || hlo != hup) return false;
  }
  const int64_t nzk = ip[n];
  // mirror positions of the upper entries
  std::vector<int32_t> mir(nzk);
  {
    const int R = std::max(1, host_threads());
    std::vector<int64_t> lowcum(n + 1, 0);
#pragma omp parallel for schedule(static)
    for (int32_t i = 0; i < n; ++i) lowcum[i + 1] = std::lower_bound(ix + ip[i], ix + ip[i + 1], i) - (ix + ip[i]);
    for (int32_t i = 0; i < n; ++i) lowcum[i + 1] += lowcum[i];
    std::vector<int32_t> cut(R + 1, n);
    cut[0] = 0;
    for (int q = 1; q < R; ++q)
      cut[q] = (int32_t)(std::lower_bound(lowcum.begin(), lowcum.end(), lowcum[n] * q / R) - lowcum.begin());
    for (int q = 1; q <= R; ++q) cut[q] = std::max(cut[q], cut[q - 1]);
#pragma omp parallel for schedule(dynamic, 1)
    for (int q = 0; q < R; ++q) {
      const int32_t i0 = cut[q], i1 = cut[q + 1];
      if (i1 <= i0) continue;
      std::vector<int32_t> cur(i1 - i0, 0);
      for (int32_t j = 0; j < i1; ++j) {  // rows j >= i1 have no upper entry below i1
        const int32_t* b = ix + ip[j];
        const int32_t* e = ix + ip[j + 1];
        const int32_t* lo = std::lower_bound(b, e, std::max(i0, j + 1));
        for (const int32_t* t = lo; t < e && *t < i1; ++t) mir[t - ix] = cur[*t - i0]++;
      }
    }
  }
  std::vector<int64_t> optr(n + 1, 0);
#pragma omp parallel for schedule(dynamic, 1024)
  for (int32_t v = 0; v < n; ++v) {
    const int32_t c = iperm[v];
    int64_t m = 0;
    for (int64_t e = ip[v]; e < ip[v + 1]; ++e) m += iperm[ix[e]] >= c;
    optr[v + 1] = m;
  }
  for (int32_t v = 0; v < n; ++v) optr[v + 1] += optr[v];
  S.val_slot[k].resize(optr[n]);
  S.val_src[k].resize(optr[n]);
#pragma omp parallel
  {
    std::vector<int32_t> pos(n, -1);
#pragma omp for schedule(dynamic, 256)
    for (int32_t v = 0; v < n; ++v) {
      const int32_t c = iperm[v];
      for (int64_t e = a.cptr[c]; e < a.cptr[c + 1]; ++e) pos[a.cidx[e]] = (int32_t)(e - a.cptr[c]);
      int64_t t = optr[v];
      for (int64_t e = ip[v]; e < ip[v + 1]; ++e) {
        const int32_t u = ix[e], r = iperm[u];
        if (r < c) continue;
        S.val_slot[k][t] = r == c ? S.pat_colptr[c] : S.pat_colptr[c] + 1 + pos[r];
        S.val_src[k][t] = u <= v ? e : ip[u] + mir[e];
        ++t;
      }
    }
  }
  return true;
}

// General inputs (one half stored, unsorted rows, duplicates):
// every stored lower entry (i, j) looks its pattern slot up: column min(new i, new j), row max, found by bisection
// in the sorted column -- independent per entry, all cores, no scatter.  (A duplicate of an entry inside one
// matrix maps to the same slot; the value upload keeps one of them.)
void value_map_general(const Analysis& a, int32_t k) {
  Symbolic& S = a.S;
  const int32_t n = a.n;
  const int64_t* ip = a.indptr[k];
  const int32_t* ix = a.indices[k];
  std::vector<int64_t> lptr(n + 1, 0);
#pragma omp parallel for schedule(static)
  for (int32_t i = 0; i < n; ++i) {
    int64_t c = 0;
    for (int64_t e = ip[i]; e < ip[i + 1]; ++e) c += ix[e] >= 0 && ix[e] <= i;
    lptr[i + 1] = c;
  }
  for (int32_t i = 0; i < n; ++i) lptr[i + 1] += lptr[i];
  S.val_slot[k].resize(lptr[n]);
  S.val_src[k].resize(lptr[n]);
#pragma omp parallel for schedule(dynamic, 256)
  for (int32_t i = 0; i < n; ++i) {
    int64_t t = lptr[i];
    const int32_t ai = a.iperm[i];
    for (int64_t e = ip[i]; e < ip[i + 1]; ++e) {
      const int32_t j = ix[e];
      if (j < 0 || j > i) continue;
      const int32_t bq = a.iperm[j];
      const int32_t c = std::min(ai, bq), r = std::max(ai, bq);
      int64_t sl = S.pat_colptr[c];
      if (r != c) {
        const int32_t* lo = a.cidx.data() + a.cptr[c];
        const int32_t* hi = a.cidx.data() + a.cptr[c + 1];
        sl += 1 + (std::lower_bound(lo, hi, r) - lo);
      }
      S.val_slot[k][t] = sl;
      S.val_src[k][t] = e;
      ++t;
    }
  }
}

void value_maps(const Analysis& a) {
  a.S.val_slot.resize(a.K);
  a.S.val_src.resize(a.K);
  for (int32_t k = 0; k < a.K; ++k) {
    if (a.S.is_diag[k]) value_map_diagonal(a, k);
    else if (!value_map_canonical(a, k)) value_map_general(a, k);
  }
}

// ---------------------------------------------------------------- 10. left-looking update schedule
void update_schedule(const Analysis& a) {
  Symbolic& S = a.S;
  const int32_t ns = S.nsuper;
  S.upd_ptr.assign(ns + 1, 0);
  for (int32_t d = 0; d < ns; ++d) for_each_target_run(a, d, [&](int32_t s, int64_t, int64_t) { S.upd_ptr[s + 1]++; });
  for (int32_t s = 0; s < ns; ++s) S.upd_ptr[s + 1] += S.upd_ptr[s];
  int64_t nu = S.upd_ptr[ns];
  S.upd_src.resize(nu);
  S.upd_p0.resize(nu);
  S.upd_p1.resize(nu);
  S.upd_jp0.resize(nu);
  std::vector<int64_t> fill(S.upd_ptr.begin(), S.upd_ptr.end() - 1);
  for (int32_t d = 0; d < ns; ++d) {  // increasing d => each target's list is in increasing descendant order
    const int64_t rb = S.sn_rowptr[d], re = S.sn_rowptr[d + 1];
    for_each_target_run(a, d, [&](int32_t s, int64_t t, int64_t t2) {
      const int64_t f = fill[s]++;
      S.upd_src[f] = d;
      S.upd_p0[f] = (int32_t)(t - rb);
      S.upd_p1[f] = (int32_t)(t2 - rb);
      S.upd_jp0[f] = (S.sn_rows[t2 - 1] - S.sn_rows[t] == (int32_t)(t2 - 1 - t)) ? S.sn_rows[t] - a.out[s].start : -1;
      const double fl = run_flops(a.out[d].end - a.out[d].start, t2 - t, re - t2);
      S.update_flops += fl;
      if (d >= S.dense_first) S.update_flops_pad += fl;
    });
  }
}

// level lists, big fronts first inside a level
void level_lists(const Analysis& a) {
  Symbolic& S = a.S;
  const int32_t ns = S.nsuper;
  S.level_ptr.assign(S.nlevels + 1, 0);
  for (int32_t s = 0; s < ns; ++s) S.level_ptr[S.sn_level[s] + 1]++;
  for (int32_t l = 0; l < S.nlevels; ++l) S.level_ptr[l + 1] += S.level_ptr[l];
  S.level_fronts.resize(ns);
  std::vector<int32_t> fill(S.level_ptr.begin(), S.level_ptr.end() - 1);
  for (int32_t s = 0; s < ns; ++s) S.level_fronts[fill[S.sn_level[s]]++] = s;
}

// ---------------------------------------------------------------- 11. target tiles (their combos are built lazily)
void target_tiles(const Analysis& a) {
  Symbolic& S = a.S;
  const int32_t ns = S.nsuper;
  const int32_t TM = a.opts.tile_rows;
  S.tile_rows = TM;
  S.tile_base.assign(ns + 1, 0);
  for (int32_t s = 0; s < ns; ++s) {
    int64_t m = S.sn_rowptr[s + 1] - S.sn_rowptr[s];
    S.tile_base[s + 1] = S.tile_base[s] + (m + TM - 1) / TM;
  }
  int64_t nt = S.tile_base[ns];
  S.tile_front.resize(nt);
  for (int32_t s = 0; s < ns; ++s)
    for (int64_t g = S.tile_base[s]; g < S.tile_base[s + 1]; ++g) S.tile_front[g] = s;
  // per-level tile lists in tile order (the update plan balances its own work items; trsm / L*R tiles cost the same)
  S.level_tile_ptr.assign(S.nlevels + 1, 0);
  for (int64_t g = 0; g < nt; ++g) S.level_tile_ptr[S.sn_level[S.tile_front[g]] + 1]++;
  for (int32_t l = 0; l < S.nlevels; ++l) S.level_tile_ptr[l + 1] += S.level_tile_ptr[l];
  S.level_tiles.resize(nt);
  {
    std::vector<int64_t> fill(S.level_tile_ptr.begin(), S.level_tile_ptr.end() - 1);
    for (int64_t g = 0; g < nt; ++g) S.level_tiles[fill[S.sn_level[S.tile_front[g]]]++] = (int32_t)g;
  }
  // per-level update-pair lists (by target level)
  S.level_pair_ptr.assign(S.nlevels + 1, 0);
  for (int32_t s = 0; s < ns; ++s) S.level_pair_ptr[S.sn_level[s] + 1] += S.upd_ptr[s + 1] - S.upd_ptr[s];
  for (int32_t l = 0; l < S.nlevels; ++l) S.level_pair_ptr[l + 1] += S.level_pair_ptr[l];
  S.level_pairs.resize(S.upd_src.size());
  std::vector<int64_t> fill(S.level_pair_ptr.begin(), S.level_pair_ptr.end() - 1);
  for (int32_t s = 0; s < ns; ++s)
    for (int64_t e = S.upd_ptr[s]; e < S.upd_ptr[s + 1]; ++e) S.level_pairs[fill[S.sn_level[s]]++] = (int32_t)e;
}

}  // namespace

Symbolic* symbolic_analyze(int32_t n, int32_t K, const int64_t* const* indptr, const int32_t* const* indices,
                           const int32_t* perm_in, const SymbolicOptions& opts_in) {
  use_host_threads();
  const AnalysisSwitches sw = read_analysis_switches();
  SymbolicOptions opts = opts_in;
  if (sw.tail_wide) opts.dense_relax_wide = *sw.tail_wide;  // flop budget of a wide tail
  std::unique_ptr<Symbolic> result(new Symbolic());
  result->n = n;
  result->K = K;
  Analysis a{n, K, indptr, indices, perm_in, opts, sw, *result};
  detect_diagonal_inputs(a);
  build_adjacency(a);
  a.lap("symmetric adjacency");
  if (!order_vertices(a)) return result.release();  // (with its `error` set)
  a.lap("ordering");
  etree_and_postorder(a);
  a.lap("etree+postorder");
  permuted_pattern(a);
  a.lap("permuted pattern");
  count_columns(a);
  a.lap("column counts");
  find_supernodes(a);
  a.lap("supernodes");
  front_row_structures(a);
  a.lap("row structures");
  select_dense_tail(a);  // may start a.recount: from here on the stages read the Analysis and write the result only
  a.lap("dense tail selection");
  pad_dense_tail(a);
  a.lap("dense tail padding");
  panel_offsets_levels_children(a);
  a.lap("offsets/levels/children");
  pattern_slot_maps(a);
  a.lap("  pattern slots -> panels");
  value_maps(a);
  a.lap("  entries -> pattern slots");
  update_schedule(a);
  level_lists(a);
  a.lap("update schedule");
  target_tiles(a);
  if (a.recount.running()) {
    a.cc = a.recount.join();
    report_column_counts(a.cc, a.S);
    a.lap("column counts of the final order (joined)");
  }
  result->colcount = std::move(a.cc);
  return result.release();
}

// Step 11b, on demand: for every 128-row tile of every target panel the list of descendant row ranges ("combos")
// that land in it.  keep_front (optional, [nsuper]) restricts the enumeration to the targets a rank owns in a
// multi-GPU run; the lists of the other tiles stay empty.
void build_tile_combos(Symbolic* S, const uint8_t* keep_front, bool skip_dense, const uint8_t* skip_desc) {
  use_host_threads();
  const int32_t ns = S->nsuper;
  const int32_t TM = S->tile_rows;
  const int64_t nt = S->tile_base[ns];
  {
    // pass 1: count combos per tile, pass 2: fill. Rows of d beyond p0 are merged against rows of s.
    std::vector<int64_t> cnt(nt + 1, 0);
    for (int pass = 0; pass < 2; ++pass) {
      std::vector<int64_t> fill;
      if (pass == 1) {
        for (int64_t g = 0; g < nt; ++g) cnt[g + 1] += cnt[g];
        S->combo_ptr.assign(cnt.begin(), cnt.end());
        S->combo_pair.resize(cnt[nt]);
        S->combo_ta.resize(cnt[nt]);
        S->combo_tb.resize(cnt[nt]);
        S->combo_ip0.resize(cnt[nt]);
        fill.assign(cnt.begin(), cnt.end() - 1);
      }
#pragma omp parallel for schedule(dynamic, 64)
      for (int32_t s = 0; s < ns; ++s) {
        if (keep_front && !keep_front[s]) continue;
        const int32_t* rs = S->sn_rows.data() + S->sn_rowptr[s];
        int64_t ms = S->sn_rowptr[s + 1] - S->sn_rowptr[s];
        for (int64_t e = S->upd_ptr[s]; e < S->upd_ptr[s + 1]; ++e) {
          int32_t d = S->upd_src[e];
          if (skip_dense && s >= S->dense_first && d >= S->dense_first) continue;
          if (skip_desc && s >= S->dense_first && skip_desc[d]) continue;
          const int32_t* rd = S->sn_rows.data() + S->sn_rowptr[d];
          int32_t md = (int32_t)(S->sn_rowptr[d + 1] - S->sn_rowptr[d]);
          int32_t t = S->upd_p0[e];
          int64_t pos = 0;
          while (t < md) {
            // position of rd[t] in rs (exists by construction): gallop from the previous position
            const int32_t* it = std::lower_bound(rs + pos, rs + ms, rd[t]);
            pos = it - rs;
            int64_t tile = pos / TM;
            int64_t tile_end_pos = std::min<int64_t>((tile + 1) * TM, ms);
            int32_t lastlabel = rs[tile_end_pos - 1];
            int32_t t2 = (int32_t)(std::upper_bound(rd + t, rd + md, lastlabel) - rd);
            int64_t g = S->tile_base[s] + tile;
            if (pass == 0) {
              cnt[g + 1]++;   // each (s) handled by exactly one thread: no race on its own tiles
            } else {
              int64_t f = fill[g]++;
              S->combo_pair[f] = (int32_t)e;
              S->combo_ta[f] = t;
              S->combo_tb[f] = t2;
              const int64_t pos_last = std::lower_bound(rs + pos, rs + ms, rd[t2 - 1]) - rs;
              S->combo_ip0[f] = (pos_last - pos == (int64_t)(t2 - 1 - t)) ? (int32_t)(pos - tile * TM) : -1;
            }
            t = t2;
          }
        }
      }
    }
  }
  S->combos_built = true;
}

// Deterministic mode, on demand: the pull schedule of the sweeps and the transposed pattern index (symbolic.h).
void build_pull_schedule(Symbolic* Sp) {
  Symbolic& S = *Sp;
  if (S.pull_built) return;
  const int32_t ns = S.nsuper;
  S.pull_seg_front.clear();
  S.pull_seg_ptr.clear();
  S.pull_front_seg.assign((size_t)ns + 1, 0);
  for (int32_t s = 0; s < ns; ++s) {
    S.pull_front_seg[(size_t)s] = (int32_t)S.pull_seg_front.size();
    int64_t e = S.upd_ptr[(size_t)s];
    const int64_t e1 = S.upd_ptr[(size_t)s + 1];
    do {
      S.pull_seg_front.push_back(s);
      S.pull_seg_ptr.push_back(e);
      e = std::min<int64_t>(e1, e + Symbolic::kPullSegPairs);
    } while (e < e1);
  }
  S.pull_front_seg[(size_t)ns] = (int32_t)S.pull_seg_front.size();
  S.pull_seg_ptr.push_back(ns > 0 ? S.upd_ptr[(size_t)ns] : 0);
  S.pull_seg_slot.assign(S.pull_seg_front.size(), -1);
  S.pull_level_ptr.assign(1, 0);
  S.pull_fold_ptr.assign(1, 0);
  S.pull_level_segs.clear();
  S.pull_fold.clear();
  S.pull_max_slots = 0;
  S.pull_group_ptr.assign(1, 0);
  int32_t slots = 0;  // slots taken in the current group of levels
  for (int32_t l = 0; l < S.nlevels; ++l) {
    int32_t need = 0;
    for (int32_t q = S.level_ptr[(size_t)l]; q < S.level_ptr[(size_t)l + 1]; ++q) {
      const int32_t s = S.level_fronts[(size_t)q];
      const int32_t ng = S.pull_front_seg[(size_t)s + 1] - S.pull_front_seg[(size_t)s];
      if (ng > 1) need += ng;
    }
    if (slots > 0 && slots + need > Symbolic::kPullSlotBudget) {
      S.pull_group_ptr.push_back(l);
      slots = 0;
    }
    for (int32_t q = S.level_ptr[(size_t)l]; q < S.level_ptr[(size_t)l + 1]; ++q) {
      const int32_t s = S.level_fronts[(size_t)q];
      const int32_t g0 = S.pull_front_seg[(size_t)s], g1 = S.pull_front_seg[(size_t)s + 1];
      for (int32_t g = g0; g < g1; ++g) {
        S.pull_level_segs.push_back(g);
        if (g1 - g0 > 1) S.pull_seg_slot[(size_t)g] = slots + (g - g0);
      }
      if (g1 - g0 > 1) {
        S.pull_fold.push_back(s);
        S.pull_fold.push_back(slots);
        S.pull_fold.push_back(g1 - g0);
        slots += g1 - g0;
      }
    }
    S.pull_max_slots = std::max(S.pull_max_slots, slots);
    S.pull_level_ptr.push_back((int64_t)S.pull_level_segs.size());
    S.pull_fold_ptr.push_back((int64_t)S.pull_fold.size() / 3);
  }
  S.pull_group_ptr.push_back(S.nlevels);
  S.pull_built = true;
}

bool build_row_index(Symbolic* Sp) {
  Symbolic& S = *Sp;
  if (S.rowidx_built) return true;
  if ((int64_t)S.pat_row.size() != S.nnz_pattern || (int64_t)S.pat_colptr.size() != (int64_t)S.n + 1) return false;
  const int32_t n = S.n;
  S.pat_rowptr.assign((size_t)n + 1, 0);
  // counting sort by row; the columns are visited in ascending order, so every row's entries come out ascending in j
  for (int32_t j = 0; j < n; ++j)
    for (int64_t e = S.pat_colptr[(size_t)j]; e < S.pat_colptr[(size_t)j + 1]; ++e) {
      const int32_t i = S.pat_row[(size_t)e];
      if (i != j) S.pat_rowptr[(size_t)i + 1]++;
    }
  for (int32_t i = 0; i < n; ++i) S.pat_rowptr[(size_t)i + 1] += S.pat_rowptr[(size_t)i];
  const int64_t cnt = S.pat_rowptr[(size_t)n];
  S.pat_rowslot.assign((size_t)cnt, 0);
  S.pat_rowcol.assign((size_t)cnt, 0);
  std::vector<int64_t> fill(S.pat_rowptr.begin(), S.pat_rowptr.end() - 1);
  for (int32_t j = 0; j < n; ++j)
    for (int64_t e = S.pat_colptr[(size_t)j]; e < S.pat_colptr[(size_t)j + 1]; ++e) {
      const int32_t i = S.pat_row[(size_t)e];
      if (i == j) continue;
      const int64_t t = fill[(size_t)i]++;
      S.pat_rowslot[(size_t)t] = e;
      S.pat_rowcol[(size_t)t] = j;
    }
  S.rowidx_built = true;
  return true;
}

}  // namespace scilmm
