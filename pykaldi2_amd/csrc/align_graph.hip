// Training graphs for forced alignment (reference bin/train_se2.py:192-199,263: kaldi.alignment.MappedAligner.align).
// Host-side work; nothing here touches the device.  csrc/align_viterbi.hip consumes the packed result.
//
// What Kaldi does [upstream knowledge: TrainingGraphCompiler::CompileGraphFromText with reorder = true, GetHTransducer,
// AddSelfLoops]: the linear word acceptor of the transcript is composed with L (disambiguation symbols removed), the
// result with the context transducer and with H (transition_scale on the forward transitions, no self-loops),
// determinized and minimized, and the self-loops are added with self_loop_scale.  The acceptor those operations define
// is built directly here, in three steps:
//
//  1. Lexicon x transcript.  Product state (L state, words consumed); an arc with output label 0 keeps the word count, an
//     arc whose output is the next word advances it.  Input labels in disambig.int count as epsilon.  After trimming,
//     input epsilons are removed in the tropical semiring (shortest epsilon distance from each node, which must be
//     acyclic), giving a weighted phone graph: node = product state entered by a phone arc (or the start), arc weight =
//     epsilon distance + the phone arc's L weight, final cost = min over the closure of distance + L final weight.
//     Kaldi determinizes LG in the log semiring; paths with the same phone string are kept apart here and the Viterbi
//     pass takes the best of them.
//  2. Context.  With window width N and central position P (tree), a phone arc becomes one HMM instance per
//     (left phone, arc, right phone) that occurs along the graph: left = phone of an arc entering its source node (0 at
//     the start), right = phone of an arc leaving its destination (0 where the utterance may end).  Supported windows:
//     N = 1; N = 2 with P = 0 or 1; N = 3 with P = 1.
//  3. H with reordered self-loops (the convention of csrc/chain_sup.hip and pk2_split_to_phones): a visit of HMM state s
//     that lasts k frames emits the transition-id of the transition out of s, then k - 1 self-loop ids of s.  The graph
//     state is therefore X(i, s, q) = "instance i, HMM state s, leaving by transition q", entered by the frame that
//     emits tid(s -> q); its self-loop emits the loop id of s.  Weights, in double and rounded to f32 once per arc:
//       self-loop   self_loop_scale * -log p_loop
//       forward     transition_scale * (-log p + log(1 - p_loop)) + self_loop_scale * -log(1 - p_loop)
//     plus the phone arc's weight on the arcs that enter an instance.  A state is final when q reaches the final HMM
//     state, its instance may end the utterance, and it then carries the phone graph node's final cost.
//
// Arcs are stored per destination state, ordered by (source, transition-id); an arc from the start state has source -1.
// Finally the graph is checked for a path of exactly T frames (status 2 when there is none).
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <unordered_map>

#include "align_internal.h"
#include "openfst_io.h"
#include "sup_model.h"

struct pk2_lexicon {
  int32_t num_states = 0, start = 0;
  std::vector<int32_t> off, dst, ilabel, olabel;    // arcs grouped by source state (file order within a state)
  std::vector<float> weight, final_cost;
  std::set<int32_t> words;
};

struct pk2_align_model {
  pk2_sup_model m;
  std::map<std::array<int32_t, 4>, int32_t> first_tid;
  std::vector<double> log_probs;
  double tscale = 1.0, lscale = 1.0;
};

namespace {

struct UttGraph {
  int32_t status = 0, T = 0;   // 0 = compiled, 2 = no path of T frames, 3 = error
  std::string error;
  std::vector<int32_t> in_off, arcx, tid, pdf, fpdf, lpdf;
  std::vector<float> w, fin;
};

std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

constexpr double kInf = std::numeric_limits<double>::infinity();

struct PhoneArc { int32_t src, dst, phone; double w; };

// Step 1: the phone graph of the transcript.  Returns an error message or "".
std::string phone_graph(const pk2_lexicon& L, const int32_t* words, int32_t nw, int32_t* num_nodes, int32_t* start_node,
                        std::vector<PhoneArc>* arcs, std::vector<double>* node_final) {
  for (int32_t j = 0; j < nw; ++j)
    if (!L.words.count(words[j])) return fmt("word id %d (position %d) is not an output label of the lexicon", words[j], j);
  const int64_t W = nw + 1;
  std::unordered_map<int64_t, int32_t> id;
  std::vector<int32_t> ps, pj;
  struct PA { int32_t src, dst, phone; float w; };
  std::vector<PA> pa;
  auto get = [&](int32_t s, int32_t j) {
    auto it = id.emplace((int64_t)s * W + j, (int32_t)ps.size());
    if (it.second) { ps.push_back(s); pj.push_back(j); }
    return it.first->second;
  };
  get(L.start, 0);
  for (size_t q = 0; q < ps.size(); ++q) {
    const int32_t s = ps[q], j = pj[q];
    for (int32_t k = L.off[s]; k < L.off[s + 1]; ++k) {
      const int32_t o = L.olabel[k];
      int32_t nj;
      if (o == 0) nj = j;
      else if (j < nw && o == words[j]) nj = j + 1;
      else continue;
      const int32_t d = get(L.dst[k], nj);
      pa.push_back({(int32_t)q, d, L.ilabel[k], L.weight[k]});
    }
  }
  const int32_t NP = (int32_t)ps.size();
  // trim: keep product states that reach a final state (every one found is reachable from the start)
  std::vector<std::vector<int32_t>> rev(NP), fwd(NP);
  for (size_t k = 0; k < pa.size(); ++k) { rev[pa[k].dst].push_back((int32_t)k); fwd[pa[k].src].push_back((int32_t)k); }
  std::vector<uint8_t> keep(NP, 0);
  std::vector<int32_t> stack;
  for (int32_t q = 0; q < NP; ++q)
    if (pj[q] == nw && std::isfinite(L.final_cost[ps[q]])) { keep[q] = 1; stack.push_back(q); }
  while (!stack.empty()) {
    const int32_t q = stack.back();
    stack.pop_back();
    for (int32_t k : rev[q])
      if (!keep[pa[k].src]) { keep[pa[k].src] = 1; stack.push_back(pa[k].src); }
  }
  if (!keep[0]) return fmt("the lexicon has no path for this transcript of %d words", nw);
  // epsilon arcs among kept states must be acyclic: topological rank by Kahn's algorithm
  std::vector<int32_t> indeg(NP, 0), rank(NP, -1), order;
  for (auto& a : pa)
    if (a.phone == 0 && keep[a.src] && keep[a.dst]) ++indeg[a.dst];
  for (int32_t q = 0; q < NP; ++q)
    if (keep[q] && indeg[q] == 0) order.push_back(q);
  for (size_t h = 0; h < order.size(); ++h) {
    rank[order[h]] = (int32_t)h;
    for (int32_t k : fwd[order[h]])
      if (pa[k].phone == 0 && keep[pa[k].dst] && --indeg[pa[k].dst] == 0) order.push_back(pa[k].dst);
  }
  int32_t nkeep = 0;
  for (int32_t q = 0; q < NP; ++q) nkeep += keep[q];
  if ((int32_t)order.size() != nkeep)
    return std::string("the lexicon has a cycle of arcs with epsilon input and epsilon output");
  // nodes: the start and every destination of a kept phone arc, numbered in product order
  std::vector<int32_t> node(NP, -1);
  node[0] = 0;
  for (auto& a : pa)
    if (a.phone != 0 && keep[a.src] && keep[a.dst]) node[a.dst] = 0;
  int32_t nn = 0;
  for (int32_t q = 0; q < NP; ++q)
    if (node[q] == 0 && keep[q]) node[q] = nn++;
    else node[q] = -1;
  *num_nodes = nn;
  *start_node = node[0];
  node_final->assign(nn, kInf);
  arcs->clear();
  std::vector<double> dist(NP, kInf);
  std::vector<int32_t> seen;
  std::vector<uint8_t> mark(NP, 0);
  for (int32_t q = 0; q < NP; ++q) {
    if (node[q] < 0) continue;
    // epsilon closure of q in topological order
    seen.assign(1, q);
    mark[q] = 1;
    for (size_t h = 0; h < seen.size(); ++h)
      for (int32_t k : fwd[seen[h]])
        if (pa[k].phone == 0 && keep[pa[k].dst] && !mark[pa[k].dst]) { mark[pa[k].dst] = 1; seen.push_back(pa[k].dst); }
    std::sort(seen.begin(), seen.end(), [&](int32_t x, int32_t y) { return rank[x] < rank[y]; });
    dist[q] = 0.0;
    std::map<std::array<int32_t, 2>, size_t> at;   // (phone, dst node) -> arc: parallel arcs keep the cheaper weight
    for (int32_t r : seen) {
      const double d = dist[r];
      if (pj[r] == nw && std::isfinite(L.final_cost[ps[r]]))
        (*node_final)[node[q]] = std::min((*node_final)[node[q]], d + (double)L.final_cost[ps[r]]);
      for (int32_t k : fwd[r]) {
        const PA& a = pa[k];
        if (!keep[a.dst]) continue;
        const double c = d + (double)a.w;
        if (a.phone == 0) {
          dist[a.dst] = std::min(dist[a.dst], c);
          continue;
        }
        auto it = at.emplace(std::array<int32_t, 2>{a.phone, node[a.dst]}, arcs->size());
        if (it.second) arcs->push_back({node[q], node[a.dst], a.phone, c});
        else if (c < (*arcs)[it.first->second].w) (*arcs)[it.first->second].w = c;
      }
    }
    for (int32_t r : seen) { dist[r] = kInf; mark[r] = 0; }
  }
  return "";
}

std::string compile_one(const pk2_align_model& am, const pk2_lexicon& L, const int32_t* words, int32_t nw, int32_t T,
                        UttGraph* g) {
  const pk2_sup_model& m = am.m;
  int32_t nn = 0, start = 0;
  std::vector<PhoneArc> parc;
  std::vector<double> nfin;
  std::string err = phone_graph(L, words, nw, &nn, &start, &parc, &nfin);
  if (!err.empty()) return err;
  // ---- step 2: context instances
  const bool useL = m.P >= 1, useR = m.N - 1 - m.P >= 1;
  std::vector<std::vector<int32_t>> left(nn), right(nn), out(nn);
  for (size_t a = 0; a < parc.size(); ++a) {
    left[parc[a].dst].push_back(parc[a].phone);
    right[parc[a].src].push_back(parc[a].phone);
    out[parc[a].src].push_back((int32_t)a);
  }
  left[start].push_back(0);
  for (int32_t v = 0; v < nn; ++v)
    if (std::isfinite(nfin[v])) right[v].push_back(0);
  for (auto* vv : {&left, &right})
    for (auto& v : *vv) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); }
  struct Inst { int32_t arc, l, r; };
  std::vector<Inst> inst;
  std::vector<int32_t> arc_inst(parc.size() + 1, 0);
  const std::vector<int32_t> none{-1};
  for (size_t a = 0; a < parc.size(); ++a) {
    arc_inst[a] = (int32_t)inst.size();
    for (int32_t l : useL ? left[parc[a].src] : none)
      for (int32_t r : useR ? right[parc[a].dst] : none) inst.push_back({(int32_t)a, l, r});
  }
  arc_inst[parc.size()] = (int32_t)inst.size();
  // ---- step 3: HMM states X(i, s, q)
  struct St { int32_t inst, s, out_dst, tid_f, tid_l, fpdf, lpdf; double fw, lw; };
  std::vector<St> st;
  std::vector<int32_t> inst_off(inst.size() + 1, 0), inst_ns(inst.size());
  std::vector<int32_t> window(m.N);
  const int32_t max_phone = (int32_t)m.phone2entry.size() - 1;
  for (size_t i = 0; i < inst.size(); ++i) {
    inst_off[i] = (int32_t)st.size();
    const int32_t p = parc[inst[i].arc].phone;
    if (p < 1 || p > max_phone || m.phone2entry[p] < 0) return fmt("phone %d of the lexicon has no HMM topology", p);
    const int32_t e = m.phone2entry[p], s0 = m.entry_off[e], ns = m.entry_off[e + 1] - s0 - 1;
    inst_ns[i] = ns;
    int32_t wpos = 0;
    if (useL) window[wpos++] = inst[i].l;
    window[wpos++] = p;
    if (useR) window[wpos++] = inst[i].r;
    for (int32_t s = 0; s < ns; ++s) {
      int32_t fp, lp;
      if (!pk2::tree_answer(m, window.data(), m.fwd_class[s0 + s], &fp) || !pk2::tree_answer(m, window.data(), m.loop_class[s0 + s], &lp))
        return fmt("the tree has no pdf for phone %d, HMM state %d in this context", p, s);
      auto ft = am.first_tid.find({p, s, fp, lp});
      if (ft == am.first_tid.end())
        return fmt("no transition-model tuple for phone %d, HMM state %d with the pdfs the tree gives", p, s);
      const int32_t q0 = m.trans_off[s0 + s], q1 = m.trans_off[s0 + s + 1];
      int32_t tid_l = 0;
      double lw = 0.0, one_minus = 0.0;
      for (int32_t q = q0; q < q1; ++q)
        if (m.trans_dst[q] == s) {
          tid_l = ft->second + (q - q0);
          const double lpl = am.log_probs[tid_l];
          lw = am.lscale * -lpl;
          one_minus = std::log1p(-std::exp(lpl));
        }
      for (int32_t q = q0; q < q1; ++q) {
        if (m.trans_dst[q] == s) continue;
        const int32_t tf = ft->second + (q - q0);
        const double fw = am.tscale * (-am.log_probs[tf] + one_minus) + am.lscale * -one_minus;
        st.push_back({(int32_t)i, s, m.trans_dst[q], tf, tid_l, fp, tid_l ? lp : fp, fw, lw});
      }
    }
  }
  inst_off[inst.size()] = (int32_t)st.size();
  const int32_t S = (int32_t)st.size();
  if (S > pk2::kAlignMaxStates) return fmt("the alignment graph has %d states, more than %d", S, pk2::kAlignMaxStates);
  struct Arc { int32_t dst, src, tid, pdf; float w; int32_t loop; };
  std::vector<Arc> arcs;
  for (int32_t x = 0; x < S; ++x)
    if (st[x].tid_l) arcs.push_back({x, x, st[x].tid_l, st[x].lpdf, (float)st[x].lw, 1});
  for (size_t i = 0; i < inst.size(); ++i) {
    const Inst& I = inst[i];
    const PhoneArc& A = parc[I.arc];
    const int32_t ns = inst_ns[i];
    for (int32_t y = inst_off[i]; y < inst_off[i + 1]; ++y) {
      if (st[y].out_dst < ns) {      // inside the instance
        for (int32_t x = inst_off[i]; x < inst_off[i + 1]; ++x)
          if (st[x].s == st[y].out_dst) arcs.push_back({x, y, st[x].tid_f, st[x].fpdf, (float)st[x].fw, 0});
        continue;
      }
      // leaving the instance: into state 0 of every instance that may follow
      for (int32_t a2 : out[A.dst]) {
        if (useR && parc[a2].phone != I.r) continue;
        for (int32_t j = arc_inst[a2]; j < arc_inst[a2 + 1]; ++j) {
          if (useL && inst[j].l != A.phone) continue;
          for (int32_t x = inst_off[j]; x < inst_off[j + 1]; ++x)
            if (st[x].s == 0) arcs.push_back({x, y, st[x].tid_f, st[x].fpdf, (float)(parc[a2].w + st[x].fw), 0});
        }
      }
    }
    if (A.src == start && (!useL || I.l == 0))
      for (int32_t x = inst_off[i]; x < inst_off[i + 1]; ++x)
        if (st[x].s == 0) arcs.push_back({x, -1, st[x].tid_f, st[x].fpdf, (float)(A.w + st[x].fw), 0});
  }
  std::stable_sort(arcs.begin(), arcs.end(), [](const Arc& a, const Arc& b) {
    return a.dst != b.dst ? a.dst < b.dst : a.src != b.src ? a.src < b.src : a.tid < b.tid;
  });
  g->in_off.assign(S + 1, 0);
  for (auto& a : arcs) ++g->in_off[a.dst + 1];
  for (int32_t x = 0; x < S; ++x) {
    if (g->in_off[x + 1] > 65535) return fmt("state %d of the alignment graph has %d in-arcs, more than 65535", x, g->in_off[x + 1]);
    g->in_off[x + 1] += g->in_off[x];
  }
  g->arcx.resize(arcs.size()); g->tid.resize(arcs.size()); g->pdf.resize(arcs.size()); g->w.resize(arcs.size());
  for (size_t k = 0; k < arcs.size(); ++k) {
    g->arcx[k] = (arcs[k].src + 1) << 1 | arcs[k].loop;
    g->tid[k] = arcs[k].tid; g->pdf[k] = arcs[k].pdf; g->w[k] = arcs[k].w;
  }
  g->fpdf.resize(S); g->lpdf.resize(S);
  g->fin.assign(S, std::numeric_limits<float>::infinity());
  for (int32_t x = 0; x < S; ++x) {
    g->fpdf[x] = st[x].fpdf; g->lpdf[x] = st[x].lpdf;
    const Inst& I = inst[st[x].inst];
    const int32_t d = parc[I.arc].dst;
    if (st[x].out_dst == inst_ns[st[x].inst] && std::isfinite(nfin[d]) && (!useR || I.r == 0)) g->fin[x] = (float)nfin[d];
  }
  // ---- a path of exactly T frames?  (the reachable set is periodic once it repeats)
  std::vector<uint8_t> cur(S, 0), nxt(S);
  for (size_t k = 0; k < arcs.size(); ++k)
    if (arcs[k].src < 0) cur[arcs[k].dst] = 1;
  for (int32_t t = 1; t < T; ++t) {
    for (int32_t x = 0; x < S; ++x) {
      uint8_t r = 0;
      for (int32_t k = g->in_off[x]; k < g->in_off[x + 1] && !r; ++k) r = arcs[k].src >= 0 && cur[arcs[k].src];
      nxt[x] = r;
    }
    if (nxt == cur) break;
    cur.swap(nxt);
  }
  bool any = false;
  for (int32_t x = 0; x < S && !any; ++x) any = cur[x] && std::isfinite(g->fin[x]);
  if (!any) {
    *g = UttGraph();
    g->status = 2;
    g->error = fmt("no path of %d frames through the alignment graph of this transcript", T);
  }
  return "";
}

pk2_lexicon* lexicon_build(int64_t ns, int64_t start, int64_t na, const int32_t* src, const int32_t* dst, const int32_t* il,
                           const int32_t* ol, const float* w, const float* fin, const int32_t* disambig, int32_t nd) {
  auto fail = [](const char* msg) -> pk2_lexicon* { pk2::set_error("pk2_lexicon: %s", msg); return nullptr; };
  if (ns < 1 || ns > (int64_t(1) << 30) || start < 0 || start >= ns || na < 0 || (na > 0 && (!src || !dst || !il || !ol || !w)) || !fin ||
      (nd > 0 && !disambig))
    return fail("bad or empty lexicon (an L.fst needs at least its start state)");
  std::set<int32_t> dis(disambig, disambig + std::max(nd, 0));
  auto* L = new pk2_lexicon;
  L->num_states = (int32_t)ns; L->start = (int32_t)start;
  L->off.assign(ns + 1, 0);
  for (int64_t k = 0; k < na; ++k) {
    if (src[k] < 0 || src[k] >= ns || dst[k] < 0 || dst[k] >= ns || il[k] < 0 || ol[k] < 0) { delete L; return fail("arc out of range"); }
    ++L->off[src[k] + 1];
  }
  for (int64_t s = 0; s < ns; ++s) L->off[s + 1] += L->off[s];
  L->dst.resize(na); L->ilabel.resize(na); L->olabel.resize(na); L->weight.resize(na);
  std::vector<int32_t> fill(L->off.begin(), L->off.end() - 1);
  for (int64_t k = 0; k < na; ++k) {
    const int32_t at = fill[src[k]]++;
    L->dst[at] = dst[k];
    L->ilabel[at] = dis.count(il[k]) ? 0 : il[k];
    L->olabel[at] = ol[k];
    L->weight[at] = w[k];
    if (ol[k] != 0) L->words.insert(ol[k]);
  }
  L->final_cost.assign(fin, fin + ns);
  return L;
}

}  // namespace

struct pk2_align_graphs {
  std::vector<UttGraph> g;
  std::vector<int32_t> packed;
  size_t ws_bytes = 0;
  int32_t max_pdf = -1, max_states = 0;
};

extern "C" {

pk2_lexicon* pk2_lexicon_create(int32_t num_states, int32_t start, int64_t num_arcs, const int32_t* src, const int32_t* dst,
                                const int32_t* ilabel, const int32_t* olabel, const float* weight, const float* final_cost,
                                const int32_t* disambig, int32_t num_disambig) {
  return lexicon_build(num_states, start, num_arcs, src, dst, ilabel, olabel, weight, final_cost, disambig, num_disambig);
}

pk2_lexicon* pk2_lexicon_from_openfst(const char* path, const int32_t* disambig, int32_t num_disambig) {
  if (!path) { pk2::set_error("pk2_lexicon_from_openfst: null path"); return nullptr; }
  pk2::FstArrays f;
  const std::string err = pk2::read_openfst(path, &f);
  if (!err.empty()) { pk2::set_error("pk2_lexicon_from_openfst: %s: %s", path, err.c_str()); return nullptr; }
  return lexicon_build(f.num_states, f.start, (int64_t)f.src.size(), f.src.data(), f.dst.data(), f.ilabel.data(),
                       f.olabel.data(), f.weight.data(), f.final_cost.data(), disambig, num_disambig);
}

void pk2_lexicon_destroy(pk2_lexicon* L) { delete L; }

pk2_align_model* pk2_align_model_create(const pk2_sup_model* m, int32_t num_tuples, const int32_t* tuples, int32_t num_tids,
                                        const double* log_probs, double transition_scale, double self_loop_scale) {
  auto fail = [](const char* msg) -> pk2_align_model* { pk2::set_error("pk2_align_model_create: %s", msg); return nullptr; };
  if (!m || num_tuples < 1 || !tuples || num_tids < 1 || !log_probs) return fail("null or empty argument");
  if (!((m->N == 1 && m->P == 0) || (m->N == 2 && (m->P == 0 || m->P == 1)) || (m->N == 3 && m->P == 1)))
    return fail("only context windows N = 1, N = 2 (P = 0 or 1) and N = 3 (P = 1) are supported");
  auto* am = new pk2_align_model;
  am->m = *m;
  am->tscale = transition_scale; am->lscale = self_loop_scale;
  am->log_probs.assign(log_probs, log_probs + num_tids + 1);
  const int32_t max_phone = (int32_t)m->phone2entry.size() - 1;
  int32_t tid = 1;
  for (int32_t i = 0; i < num_tuples; ++i) {
    const int32_t* t = tuples + 4 * i;
    if (t[0] < 1 || t[0] > max_phone || m->phone2entry[t[0]] < 0) { delete am; return fail("tuple of a phone without topology"); }
    const int32_t e = m->phone2entry[t[0]], s = m->entry_off[e] + t[1];
    if (t[1] < 0 || s >= m->entry_off[e + 1] - 1) { delete am; return fail("tuple of a non-emitting HMM state"); }
    am->first_tid[{t[0], t[1], t[2], t[3]}] = tid;
    tid += m->trans_off[s + 1] - m->trans_off[s];
  }
  if (tid - 1 != num_tids) { delete am; return fail("the tuples enumerate a different number of transition-ids than log_probs holds"); }
  return am;
}

void pk2_align_model_destroy(pk2_align_model* am) { delete am; }

pk2_align_graphs* pk2_align_compile(const pk2_align_model* am, const pk2_lexicon* L, int32_t num_utts, const int32_t* word_off,
                                    const int32_t* words, const int32_t* frames) {
  if (!am || !L || num_utts < 1 || !word_off || !frames || (word_off[num_utts] > 0 && !words)) {
    pk2::set_error("pk2_align_compile: bad argument");
    return nullptr;
  }
  auto* G = new pk2_align_graphs;
  G->g.resize(num_utts);
  for (int32_t n = 0; n < num_utts; ++n) {
    UttGraph& g = G->g[n];
    const int32_t T = frames[n], nw = word_off[n + 1] - word_off[n];
    std::string err = T < 1 ? fmt("utterance of %d frames", T) : nw < 0 ? std::string("bad word offsets")
                                                                        : compile_one(*am, *L, words + word_off[n], nw, T, &g);
    if (!err.empty()) { g = UttGraph(); g.status = 3; g.error = err; }
    g.T = std::max(T, 0);
    for (int32_t p : g.pdf) G->max_pdf = std::max(G->max_pdf, p);
    G->max_states = std::max(G->max_states, (int32_t)g.fpdf.size());
  }
  // pack: descriptors, then the arrays of each utterance on 16-word boundaries; workspace offsets per utterance
  auto up16 = [](size_t x) { return (x + 15) / 16 * 16; };
  size_t words_total = up16((size_t)num_utts * 16);
  std::vector<pk2::AlignDesc> desc(num_utts);
  size_t ws = 0;
  for (int32_t n = 0; n < num_utts; ++n) {
    UttGraph& g = G->g[n];
    pk2::AlignDesc& d = desc[n];
    const int32_t S = (int32_t)g.fpdf.size(), A = (int32_t)g.arcx.size();
    d = pk2::AlignDesc{S, A, g.T, g.status, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int32_t* fields[8] = {&d.in_off, &d.arcx, &d.w, &d.tid, &d.pdf, &d.fpdf, &d.lpdf, &d.fin};
    const size_t sizes[8] = {(size_t)S + 1, (size_t)A, (size_t)A, (size_t)A, (size_t)A, (size_t)S, (size_t)S, (size_t)S};
    for (int f = 0; f < 8; ++f) { *fields[f] = (int32_t)words_total; words_total += up16(sizes[f]); }
    if (S > 0) {
      d.bp = (int64_t)ws;
      ws += pk2::align_up((size_t)g.T * S * 4, 256);
      d.scr = (int64_t)ws;
      ws += pk2::align_up(((size_t)2 * S + 2 * (size_t)g.T) * 4, 256);
    }
  }
  if (words_total > (size_t)INT32_MAX) { delete G; pk2::set_error("pk2_align_compile: packed graphs exceed 2^31 words"); return nullptr; }
  G->packed.assign(words_total, 0);
  std::memcpy(G->packed.data(), desc.data(), sizeof(pk2::AlignDesc) * num_utts);
  for (int32_t n = 0; n < num_utts; ++n) {
    const UttGraph& g = G->g[n];
    const pk2::AlignDesc& d = desc[n];
    auto put = [&](int32_t at, const void* src, size_t count) { if (count) std::memcpy(G->packed.data() + at, src, 4 * count); };
    if (d.S == 0) continue;
    put(d.in_off, g.in_off.data(), g.in_off.size()); put(d.arcx, g.arcx.data(), g.arcx.size());
    put(d.w, g.w.data(), g.w.size()); put(d.tid, g.tid.data(), g.tid.size()); put(d.pdf, g.pdf.data(), g.pdf.size());
    put(d.fpdf, g.fpdf.data(), g.fpdf.size()); put(d.lpdf, g.lpdf.data(), g.lpdf.size()); put(d.fin, g.fin.data(), g.fin.size());
  }
  G->ws_bytes = ws + 256;
  return G;
}

void pk2_align_graphs_destroy(pk2_align_graphs* G) { delete G; }

int pk2_align_graphs_info(const pk2_align_graphs* G, int32_t utt, int32_t* status, int32_t* num_states, int32_t* num_arcs) {
  PK2_REQUIRE(G && utt >= 0 && utt < (int32_t)G->g.size(), "pk2_align_graphs_info: bad argument");
  const UttGraph& g = G->g[utt];
  if (status) *status = g.status;
  if (num_states) *num_states = (int32_t)g.fpdf.size();
  if (num_arcs) *num_arcs = (int32_t)g.arcx.size();
  return PK2_OK;
}

const char* pk2_align_graphs_error(const pk2_align_graphs* G, int32_t utt) {
  if (!G || utt < 0 || utt >= (int32_t)G->g.size()) return "";
  return G->g[utt].error.c_str();
}

int pk2_align_graphs_copy(const pk2_align_graphs* G, int32_t utt, int32_t* in_off, int32_t* arc_src, int32_t* arc_tid,
                          int32_t* arc_pdf, float* arc_weight, float* final_cost) {
  PK2_REQUIRE(G && utt >= 0 && utt < (int32_t)G->g.size(), "pk2_align_graphs_copy: bad argument");
  const UttGraph& g = G->g[utt];
  auto put = [](auto* out, const auto& v) { if (out) std::copy(v.begin(), v.end(), out); };
  put(in_off, g.in_off); put(arc_tid, g.tid); put(arc_pdf, g.pdf); put(arc_weight, g.w); put(final_cost, g.fin);
  if (arc_src)
    for (size_t k = 0; k < g.arcx.size(); ++k) arc_src[k] = (g.arcx[k] >> 1) - 1;
  return PK2_OK;
}

int64_t pk2_align_graphs_packed_words(const pk2_align_graphs* G) { return G ? (int64_t)G->packed.size() : 0; }

int pk2_align_graphs_pack(const pk2_align_graphs* G, int32_t* out) {
  PK2_REQUIRE(G && out, "pk2_align_graphs_pack: null argument");
  std::memcpy(out, G->packed.data(), 4 * G->packed.size());
  return PK2_OK;
}

size_t pk2_align_workspace_bytes(const pk2_align_graphs* G) { return G ? G->ws_bytes : 0; }

}  // extern "C"

// Read by csrc/align_viterbi.hip.
namespace pk2 {
void align_graphs_limits(const pk2_align_graphs* G, int32_t* num_utts, int32_t* max_states, int32_t* max_pdf, int32_t* max_arcs,
                         size_t* ws_bytes, const int32_t** packed) {
  *num_utts = (int32_t)G->g.size();
  *max_states = G->max_states;
  *max_pdf = G->max_pdf;
  int32_t a = 0;
  for (auto& g : G->g) a = std::max(a, (int32_t)g.arcx.size());
  *max_arcs = a;
  *ws_bytes = G->ws_bytes;
  *packed = G->packed.data();
}
}  // namespace pk2
