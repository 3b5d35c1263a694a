// mrk_plan.cpp -- the query planner: mrk_query (flattened XQNode_t tree + ranker knobs) -> device passes and work
// items.  Mirrors what sphCreateRanker / ExtNode_i::Create decide on the host in the reference
// (sphinxsearch.cpp:4167-4378, searchnode.cpp:1599-1811).
#include "mrk_host_int.h"
#include "mrk_sortkey.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <optional>

using namespace mrk;

// Fixed-capacity vector for the planner's scratch lists: planning runs per query on the submit path (a few hundred
// nanoseconds each), heap allocations would dominate it.  Pushing past the capacity sets `overflow` (checked once per
// query: such a query is declined) instead of growing.
template <typename T, int N>
struct SmallVec {
  T v[N];
  int n = 0;
  bool overflow = false;
  SmallVec() {}
  explicit SmallVec(int count) : n(count <= N ? count : N), overflow(count > N) {
    for (int i = 0; i < n; ++i) v[i] = T();
  }
  void push_back(const T& x) {
    if (n < N)
      v[n++] = x;
    else
      overflow = true;
  }
  size_t size() const { return (size_t)n; }
  bool empty() const { return n == 0; }
  T& operator[](size_t i) { return v[i]; }
  const T& operator[](size_t i) const { return v[i]; }
  T* begin() { return v; }
  T* end() { return v + n; }
  const T* begin() const { return v; }
  const T* end() const { return v + n; }
  T& back() { return v[n - 1]; }
  const T& back() const { return v[n - 1]; }
  T& front() { return v[0]; }
  const T& front() const { return v[0]; }
  void clear() { n = 0; }
  void append(const T* b, const T* e) {
    for (; b != e; ++b) push_back(*b);
  }
};
constexpr int PLAN_CAP = 40; // keywords / nodes / children a plan may hold before the size checks decline the query
typedef SmallVec<int, PLAN_CAP> IntVec;

// planner: mrk_query -> DevQuery + work items
// ----------------------------------------------------------------------------------------
struct PlanKw { // one keyword occurrence of the query tree
  int32_t term_id;
  int32_t node;
  int docs;
  float boost, idf;
  uint32_t queried32;
  int atom_pos;
  int tp_kind, tp_max; // MRK_TERMPOS_*
  bool weighted_first; // first node of its word in GetQwords order gets the IDF, later dupes get 0
  bool hidden = false; // the boundary keyword of a SENTENCE / PARAGRAPH node: read for its hits, not a query word (bNotWeighted, no IDF, no query position)
};

struct PlanNode { // binary eval-tree node, post-order
  uint32_t op;
  int l = -1, r = -1, kw = -1;
};

struct PlanTree {
  SmallVec<PlanKw, PLAN_CAP> kws;     // in GetQwords traversal order
  SmallVec<PlanNode, PLAN_CAP> nodes; // post-order; root = last
  bool multiand3_inner = false; // a 3-keyword ExtMultiAnd_T below the root (MergeHits3 quirk not restated there)
  bool phrase = false;          // root is a PHRASE (ExtNWay_T<FSMphrase_c>)
  bool ph_leaf = false;         // one PHRASE below other operators; its words are kws[ph_kw0 .. ph_kw0 + ph_n)
  int ph_kw0 = 0, ph_n = 0;
  int px_dist = 0;              // > 0: the phrase node is a PROXIMITY operator ('"a b"~N')
  bool force_tree = false;      // the query must run as a tree program even if it only holds TERM / AND nodes
  // one real ExtQuorum_c ('"a b c"/N', 1 < N < words): its keywords are kws[q_kw0 .. q_kw0 + q_n) in query-position order
  bool quorum = false, quorum_root = false;
  bool order = false;           // the ph_leaf node is a BEFORE operator (ExtOrder_c), not a PHRASE
  bool termpos = false;         // some keyword carries a position modifier ('^word', 'word$', '@field[N] word')
  bool notnear = false;         // one NOTNEAR node over two plain keywords: kws[nn_a] NOTNEAR/nn_dist kws[nn_b]
  int nn_a = 0, nn_b = 0, nn_dist = 0;
  int q_kw0 = 0, q_n = 0, q_thr = 0;
  IntVec atoms;                 // its words' query positions, phrase order
  bool gen_nearn = false;       // ... with a NEAR over three and more operands at its root
  bool gen = false;             // planned for the generic per-doc evaluator: nodes = the doc-level superset tree, the real tree is a GenProg
};

// Mirrors ExtNode_i::Create (searchnode.cpp:1599-1811) for the operators the device path knows:
// AND over plain keywords -> ExtMultiAnd_T (nodes sorted by ascending docs with sphSort's small-array
// insertion sort, sphinxstd.h:853-869: equal keys end in reverse arrival order); other AND / OR / MAYBE /
// ANDNOT -> left-deep chains in child order (searchnode.cpp:1785-1806).  An N-way MultiAnd is emitted as
// a left-deep AND chain: ((0+t0)+t1)+t2 and (t0+t1)+t2 are the same fp32 value.
static int build_tree(const mrk_segment* seg, const mrk_query& q, int32_t ni, PlanTree& T, uint32_t qi, int depth, bool is_root, int& err) {
  if (ni < 0 || ni >= q.n_nodes || depth > 16) return err = mrk_fail(MRK_E_INVAL, "query %u: bad tree", qi), -1;
  const mrk_node& n = q.nodes[ni];
  auto leaf = [&](int32_t li) -> int {
    const mrk_node& t = q.nodes[li];
    PlanKw k{};
    k.term_id = t.term_id;
    k.node = li;
    k.docs = (t.term_id >= 0 && (uint32_t)t.term_id < seg->terms.size()) ? (int)seg->terms[t.term_id].docs : 0;
    k.boost = t.boost;
    k.queried32 = t.field_mask;
    k.atom_pos = t.atom_pos;
    k.tp_kind = t.term_pos;
    k.tp_max = t.field_max_pos;
    if (t.term_pos) T.termpos = T.force_tree = true; // ExtTermPos_T never sits inside an ExtMultiAnd_T (searchnode.cpp:1724-1735)
    T.kws.push_back(k);
    PlanNode pn;
    pn.op = PN_TERM;
    pn.kw = (int)T.kws.size() - 1;
    T.nodes.push_back(pn);
    return (int)T.nodes.size() - 1;
  };
  auto join = [&](uint32_t op, int l, int r) -> int {
    PlanNode pn;
    pn.op = op;
    pn.l = l;
    pn.r = r;
    T.nodes.push_back(pn);
    return (int)T.nodes.size() - 1;
  };
  if (n.op == MRK_OP_TERM) return leaf(ni);
  const bool near = n.op == MRK_OP_NEAR; // ExtNWay_T<FSMmultinear_c>: the same node with a third state machine
  const bool nway = n.op == MRK_OP_PHRASE || n.op == MRK_OP_PROXIMITY || near; // ExtNWay_T<FSMphrase_c / FSMproximity_c / FSMmultinear_c>
  if (nway && (T.phrase || T.ph_leaf))
    return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: more than one PHRASE (device path: one per query)", qi), -1;
  if (n.op == MRK_OP_QUORUM) {
    // ExtNode_i::Create, SPH_QUERY_QUORUM (searchnode.cpp:1638-1686): threshold 1 = an ExtOr_c chain, threshold >= word
    // count = an ExtAnd_c chain, both over the words sorted by ascending doc count; a real ExtQuorum_c in between
    if (n.n_children < 2 || n.n_children > 16 || n.first_child < 0) return err = mrk_fail(MRK_E_INVAL, "query %u: bad child list", qi), -1;
    if (n.opt < 1) return err = mrk_fail(MRK_E_INVAL, "query %u: quorum threshold %d", qi, n.opt), -1;
    const bool real_quorum = n.opt != 1 && n.opt < n.n_children;
    if (real_quorum && (T.quorum || n.n_children > QUORUM_EVENTS))
      return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: quorum nodes on the device path: one per query, <= %d keywords", qi, QUORUM_EVENTS), -1;
    IntVec kids(n.n_children), ord(n.n_children), docs(n.n_children);
    for (int i = 0; i < n.n_children; ++i) {
      kids[i] = q.children[n.first_child + i];
      if (kids[i] < 0 || kids[i] >= q.n_nodes || q.nodes[kids[i]].op != MRK_OP_TERM || q.nodes[kids[i]].term_pos)
        return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: quorum over plain keywords only", qi), -1;
      const mrk_node& t = q.nodes[kids[i]];
      docs[i] = (t.term_id >= 0 && (uint32_t)t.term_id < seg->terms.size()) ? (int)seg->terms[t.term_id].docs : 0;
      ord[i] = i;
    }
    for (int i = 1; i < n.n_children; ++i)
      for (int j = i; j > 0; --j) {
        if (docs[ord[j - 1]] < docs[ord[j]]) break;
        std::swap(ord[j], ord[j - 1]);
      }
    const size_t kw0 = T.kws.size();
    if (real_quorum) {
      // ExtQuorum_c (searchnode.cpp:4342-4403): children in query-position order, no TERM nodes of their own in the
      // program -- the node reads its keywords' presence bits itself
      for (int i = 0; i < n.n_children; ++i) ord[i] = i;
      std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return q.nodes[kids[a]].atom_pos < q.nodes[kids[b]].atom_pos; });
      const size_t nodes0 = T.nodes.size();
      for (int i = 0; i < n.n_children; ++i) {
        for (int j = 0; j < i; ++j)
          if (q.nodes[kids[ord[i]]].term_id >= 0 && q.nodes[kids[ord[j]]].term_id == q.nodes[kids[ord[i]]].term_id)
            return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: quorum with a repeated keyword (m_bHasDupes) is not on the device path", qi), -1;
        (void)leaf(kids[ord[i]]);
      }
      T.nodes.n = (int)nodes0; // drop the TERM nodes leaf() appended; the keywords stay in T.kws
      for (size_t k = kw0; k < T.kws.size(); ++k) {
        T.kws[k].queried32 &= n.field_mask;
        // where a keyword's stream ends is only known for unrestricted keywords (its last doc); see qr_row
        const uint32_t all = seg->n_fields >= 32 ? 0xFFFFFFFFu : (1u << seg->n_fields) - 1u;
        if ((T.kws[k].queried32 & all) != all)
          return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: field-limited keywords in a quorum are not on the device path", qi), -1;
      }
      T.quorum = true;
      T.quorum_root = is_root;
      T.q_kw0 = (int)kw0;
      T.q_n = n.n_children;
      T.q_thr = n.opt;
      PlanNode pn;
      pn.op = PN_QUORUM;
      T.nodes.push_back(pn);
      return (int)T.nodes.size() - 1;
    }
    int cur = leaf(kids[ord[0]]);
    for (int i = 1; i < n.n_children; ++i) {
      const int r = leaf(kids[ord[i]]);
      cur = join(n.opt == 1 ? PN_OR : PN_AND, cur, r);
    }
    for (size_t k = kw0; k < T.kws.size(); ++k) T.kws[k].queried32 &= n.field_mask; // Create ( word, pNode, .. )
    T.force_tree = true; // an ExtAnd_c chain is not an ExtMultiAnd_T (no MergeHits3 quirk): always the tree program
    return cur;
  }
  if (n.op == MRK_OP_NOTNEAR) {
    // ExtNotNear_c (generic create, searchnode.cpp:1785-1803): the must side's docs; where the not side holds the doc too, only
    // the must hits no later not-hit comes within the distance of survive, and the doc stays iff one does
    if (T.notnear || T.phrase || T.ph_leaf || T.order)
      return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: NOTNEAR next to another NOTNEAR / PHRASE / BEFORE node (device path: one such node per query)", qi), -1;
    if (n.n_children != 2 || n.first_child < 0) return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: NOTNEAR over %d operands (device path: two plain keywords)", qi, n.n_children), -1;
    if (n.opt <= 0 || n.opt > (1 << 20)) return err = mrk_fail(MRK_E_INVAL, "query %u: NOTNEAR distance %d", qi, n.opt), -1;
    int kid[2];
    for (int i = 0; i < 2; ++i) {
      kid[i] = q.children[n.first_child + i];
      if (kid[i] < 0 || kid[i] >= q.n_nodes) return err = mrk_fail(MRK_E_INVAL, "query %u: child index out of range", qi), -1;
      if (q.nodes[kid[i]].op != MRK_OP_TERM || q.nodes[kid[i]].term_pos)
        return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: NOTNEAR over plain keywords only on the device path", qi), -1;
    }
    const int l = leaf(kid[0]);
    T.nn_a = (int)T.kws.size() - 1;
    const int r = leaf(kid[1]);
    T.nn_b = (int)T.kws.size() - 1;
    T.nn_dist = n.opt;
    T.notnear = T.force_tree = true;
    return join(PN_NOTNEAR, l, r);
  }
  if (n.op == MRK_OP_BEFORE) {
    // ExtOrder_c (CreateOrderNode, searchnode.cpp:1044-1073): children in query order, no sorting; the doc is the FIRST
    // child's doc (fields, tfidf) once all children hold it and their hits line up in order inside one field
    if (T.phrase || T.ph_leaf)
      return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: more than one PHRASE / BEFORE node (device path: one per query)", qi), -1;
    if (n.n_children < 2 || n.n_children > MAX_PROX_TERMS || n.first_child < 0)
      return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: BEFORE over %d nodes (device path: 2..%d plain keywords)", qi, n.n_children, MAX_PROX_TERMS), -1;
    const int kw0 = (int)T.kws.size();
    int cur = -1;
    for (int i = 0; i < n.n_children; ++i) {
      const int32_t ki = q.children[n.first_child + i];
      if (ki < 0 || ki >= q.n_nodes) return err = mrk_fail(MRK_E_INVAL, "query %u: child index out of range", qi), -1;
      if (q.nodes[ki].op != MRK_OP_TERM)
        return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: BEFORE over plain keywords only on the device path", qi), -1;
      T.atoms.push_back(q.nodes[ki].atom_pos);
      if (i && T.atoms[i] <= T.atoms[i - 1]) return err = mrk_fail(MRK_E_INVAL, "query %u: BEFORE operands' query positions must ascend", qi), -1;
      const int l = leaf(ki);
      cur = cur < 0 ? l : join(PN_AND, cur, l);
    }
    T.ph_leaf = T.order = T.force_tree = true;
    T.ph_kw0 = kw0;
    T.ph_n = n.n_children;
    PlanNode pn;
    pn.op = PN_ORDERFIX;
    pn.l = cur;
    pn.kw = kw0; // the first child: its doc is the node's doc
    T.nodes.push_back(pn);
    return (int)T.nodes.size() - 1;
  }
  if (!nway && n.op != MRK_OP_AND && n.op != MRK_OP_OR && n.op != MRK_OP_MAYBE && n.op != MRK_OP_ANDNOT)
    return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: operator %d not on the device path yet", qi, n.op), -1;
  if (n.n_children < 1 || n.n_children > 16 || n.first_child < 0) return err = mrk_fail(MRK_E_INVAL, "query %u: bad child list", qi), -1;
  IntVec kids(n.n_children);
  bool all_terms = true;
  for (int i = 0; i < n.n_children; ++i) {
    kids[i] = q.children[n.first_child + i];
    if (kids[i] < 0 || kids[i] >= q.n_nodes) return err = mrk_fail(MRK_E_INVAL, "query %u: child index out of range", qi), -1;
    all_terms &= q.nodes[kids[i]].op == MRK_OP_TERM;
  }
  if (nway) {
    if (n.op == MRK_OP_PROXIMITY || near) {
      if (n.opt <= 0 || n.opt > (1 << 20)) return err = mrk_fail(MRK_E_INVAL, "query %u: proximity / NEAR distance %d", qi, n.opt), -1;
      T.px_dist = n.opt | (near ? (int)0x80000000u : 0);
    }
    // NEAR: two plain keywords on the device.  With three or more operands the reference's folded hit carries a query position
    // that depends on the docs evaluated before (FSMmultinear_c::m_uFirstQpos is never reset for the ring form), and operands
    // that are phrases / groups need their own hit streams: both are declined
    if (near && (!all_terms || n.n_children != 2))
      return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: NEAR over %d operands (device path: two plain keywords)", qi, n.n_children), -1;
    // CreateMultiNode<ExtPhrase_c / ExtProximity_c> (searchnode.cpp:984-1041): plain keywords only; ExtNWay_T::ConstructNode
    // (:3767-3787) chains them left-deep in ascending doc-count order, so docs / tfidf come out as for a MultiAnd
    if (!all_terms || n.n_children < 2 || n.n_children > MAX_PROX_TERMS)
      return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: PHRASE of %d nodes (device path: 2..%d plain keywords)", qi, n.n_children,
                            MAX_PROX_TERMS), -1;
    (is_root ? T.phrase : T.ph_leaf) = true;
    for (int i = 0; i < n.n_children; ++i) {
      T.atoms.push_back(q.nodes[kids[i]].atom_pos);
      if (i && T.atoms[i] <= T.atoms[i - 1]) return err = mrk_fail(MRK_E_INVAL, "query %u: phrase atom positions must ascend", qi), -1;
    }
    if (!near && T.atoms.back() - T.atoms.front() >= PHRASE_STATES)
      return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: phrase spans %d positions (device path: < %d)", qi,
                            T.atoms.back() - T.atoms.front(), PHRASE_STATES), -1;
  }
  if ((n.op == MRK_OP_AND || nway) && all_terms && n.n_children > 1) {
    IntVec ord(n.n_children), docs(n.n_children);
    bool any_tp = false;
    for (int i = 0; i < n.n_children; ++i) {
      const mrk_node& t = q.nodes[kids[i]];
      docs[i] = (t.term_id >= 0 && (uint32_t)t.term_id < seg->terms.size()) ? (int)seg->terms[t.term_id].docs : 0;
      ord[i] = i;
      if (t.term_pos) { // ExtConditional_T keeps ExtNode_i's GetDocsCount() = INT_MAX (searchnode.h:83): sorted last
        if (nway) return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: position modifiers on the words of a phrase", qi), -1;
        docs[i] = INT_MAX;
        any_tp = true;
      }
    }
    for (int i = 1; i < n.n_children; ++i)
      for (int j = i; j > 0; --j) {
        if (docs[ord[j - 1]] < docs[ord[j]]) break;
        std::swap(ord[j], ord[j - 1]);
      }
    if (n.op == MRK_OP_AND && n.n_children == 3 && !is_root && !any_tp) T.multiand3_inner = true;
    const int kw0 = (int)T.kws.size();
    int cur = leaf(kids[ord[0]]);
    for (int i = 1; i < n.n_children; ++i) {
      const int r = leaf(kids[ord[i]]);
      cur = join(PN_AND, cur, r);
    }
    if (nway) { // the words are created with the phrase node's field limit (searchnode.cpp:1020-1024)
      for (size_t k = (size_t)kw0; k < T.kws.size(); ++k) T.kws[k].queried32 &= n.field_mask;
      if (!is_root) { // ExtNWay_T on top of the words' AND chain: keeps the docs where the words line up
        T.ph_kw0 = kw0;
        T.ph_n = n.n_children;
        PlanNode pn;
        pn.op = PN_PHRASEFIX;
        pn.l = cur;
        T.nodes.push_back(pn);
        cur = (int)T.nodes.size() - 1;
      }
    }
    return cur;
  }
  const uint32_t op = n.op == MRK_OP_AND ? PN_AND : n.op == MRK_OP_OR ? PN_OR : n.op == MRK_OP_MAYBE ? PN_MAYBE : PN_ANDNOT;
  int cur = -1;
  for (int i = 0; i < n.n_children; ++i) {
    const int c = build_tree(seg, q, kids[i], T, qi, depth + 1, false, err);
    if (c < 0) return -1;
    cur = cur < 0 ? c : join(op, cur, c);
  }
  return cur;
}


// ---- the generic path: the reference's evaluation tree as a GenProg (mrk_keval.h evaluates it per candidate doc), plus
// the doc-level superset tree the scan kernel runs to find the candidates: every PHRASE / PROXIMITY / NEAR / BEFORE node as
// the AND of its operands, NOTNEAR / ANDNOT as their left side (MAYBE: the right side's keywords are still located).
// Follows ExtNode_i::Create (searchnode.cpp:1599-1811) node for node; keywords enter T.kws in GetQwords traversal order.
struct GenBuild {
  mrk::GenProg prog;
  int plan[mrk::GEN_MAX_NODES]; // the superset tree's node for each program node
  int docs[mrk::GEN_MAX_NODES]; // GetDocsCount(): a plain keyword's docs, INT_MAX for everything else (searchnode.h:83)
  int atom[mrk::GEN_MAX_NODES]; // GetAtomPos()
  bool overflow = false;
  GenBuild() { memset(&prog, 0, sizeof prog); }
  int add(const mrk::GenNode& n, int plan_node, int ndocs, int natom) {
    if (prog.n_nodes >= (uint32_t)mrk::GEN_MAX_NODES) {
      overflow = true;
      return 0;
    }
    const int i = (int)prog.n_nodes++;
    prog.nodes[i] = n;
    plan[i] = plan_node, docs[i] = ndocs, atom[i] = natom;
    return i;
  }
};

static int node_docs_key(const mrk_segment* seg, const mrk_node& t) { // what ExtNodeTF(Ext)_fn sorts operands by
  if (t.op != MRK_OP_TERM || t.term_pos) return INT_MAX;
  return (t.term_id >= 0 && (uint32_t)t.term_id < seg->terms.size()) ? (int)seg->terms[t.term_id].docs : 0;
}

static void sph_isort(IntVec& ord, const IntVec& key) { // sphSort's small-array path: equal keys end in reverse arrival order
  for (int i = 1; i < (int)ord.size(); ++i)
    for (int j = i; j > 0; --j) {
      if (key[ord[j - 1]] < key[ord[j]]) break;
      std::swap(ord[j], ord[j - 1]);
    }
}

static int build_gen(const mrk_segment* seg, const mrk_query& q, int32_t ni, PlanTree& T, GenBuild& G, uint32_t qi, int depth, int& err) {
  using namespace mrk;
  if (ni < 0 || ni >= q.n_nodes || depth > 16) return err = mrk_fail(MRK_E_INVAL, "query %u: bad tree", qi), -1;
  const mrk_node& n = q.nodes[ni];
  auto pjoin = [&](uint32_t op, int l, int r) -> int {
    PlanNode pn;
    pn.op = op, pn.l = l, pn.r = r;
    T.nodes.push_back(pn);
    return (int)T.nodes.size() - 1;
  };
  // a keyword: its slot in T.kws + its PN_TERM node in the superset tree
  auto keyword = [&](int32_t li, uint32_t mask_and, int& plan_node) -> int {
    const mrk_node& t = q.nodes[li];
    PlanKw k{};
    k.term_id = t.term_id;
    k.node = li;
    k.docs = (t.term_id >= 0 && (uint32_t)t.term_id < seg->terms.size()) ? (int)seg->terms[t.term_id].docs : 0;
    k.boost = t.boost;
    k.queried32 = t.field_mask & mask_and;
    k.atom_pos = t.atom_pos;
    k.tp_kind = t.term_pos;
    k.tp_max = t.field_max_pos;
    T.kws.push_back(k);
    PlanNode pn;
    pn.op = PN_TERM;
    pn.kw = (int)T.kws.size() - 1;
    T.nodes.push_back(pn);
    plan_node = (int)T.nodes.size() - 1;
    return pn.kw;
  };
  auto term_node = [&](int32_t li, uint32_t mask_and) -> int {
    int pl;
    const int slot = keyword(li, mask_and, pl);
    GenNode g{};
    g.kind = GN_TERM;
    g.kid[0] = (uint8_t)slot;
    return G.add(g, pl, node_docs_key(seg, q.nodes[li]), q.nodes[li].atom_pos);
  };
  auto twofer = [&](uint32_t kind, uint32_t pop, int l, int r, int opt = 0) -> int {
    GenNode g{};
    g.kind = (uint8_t)kind, g.n_kids = 2, g.kid[0] = (uint8_t)l, g.kid[1] = (uint8_t)r, g.opt = opt;
    return G.add(g, pjoin(pop, G.plan[l], G.plan[r]), INT_MAX, G.atom[l]);
  };
  // ExtNWay_T::ConstructNode (:3767-3802): the operands chained left-deep in ascending doc-count order, every hit relabelled
  // with its operand's place in the query (1-based), the last ExtAnd_c emitting in reverse query-position order.  One
  // operand at a time (operand, AND, operand, AND ...: the superset tree's program stays two values deep)
  auto nway_step = [&](int& cur, int c, const IntVec& ord, int i) {
    if (i == 0) {
      cur = c;
      return;
    }
    const int a = twofer(GN_AND, PN_AND, cur, c);
    G.prog.nodes[a].npl = (uint16_t)(i == 1 ? ord[0] + 1 : 0), G.prog.nodes[a].npr = (uint16_t)(ord[i] + 1);
    if (i + 1 == (int)ord.size()) G.prog.nodes[a].flags |= 1u;
    cur = a;
  };
  if (n.op == MRK_OP_TERM) {
    if (n.term_pos < 0 || n.term_pos > MRK_TERMPOS_LIMIT || (n.term_pos == MRK_TERMPOS_LIMIT && n.field_max_pos <= 0))
      return err = mrk_fail(MRK_E_INVAL, "query %u: bad position modifier", qi), -1;
    return term_node(ni, 0xFFFFFFFFu);
  }
  if (n.n_children < 1 || n.n_children > 16 || n.first_child < 0) return err = mrk_fail(MRK_E_INVAL, "query %u: bad child list", qi), -1;
  IntVec kids(n.n_children);
  bool all_terms = true, any_tp = false;
  for (int i = 0; i < n.n_children; ++i) {
    kids[i] = q.children[n.first_child + i];
    if (kids[i] < 0 || kids[i] >= q.n_nodes) return err = mrk_fail(MRK_E_INVAL, "query %u: child index out of range", qi), -1;
    all_terms &= q.nodes[kids[i]].op == MRK_OP_TERM;
    any_tp |= q.nodes[kids[i]].op == MRK_OP_TERM && q.nodes[kids[i]].term_pos != 0;
  }
  IntVec ord(n.n_children), key(n.n_children);
  for (int i = 0; i < n.n_children; ++i) ord[i] = i, key[i] = node_docs_key(seg, q.nodes[kids[i]]);
  switch (n.op) {
    case MRK_OP_PHRASE:
    case MRK_OP_PROXIMITY: { // CreateMultiNode<ExtPhrase_c / ExtProximity_c> (:984-1041): plain keywords under the node's field limit
      if (!all_terms || any_tp || n.n_children < 2 || n.n_children > MRK_MAX_AND_TERMS)
        return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: PHRASE of %d nodes (generic path: 2..%d plain keywords)", qi, n.n_children, MRK_MAX_AND_TERMS), -1;
      if (n.op == MRK_OP_PROXIMITY && (n.opt <= 0 || n.opt > (1 << 20))) return err = mrk_fail(MRK_E_INVAL, "query %u: proximity distance %d", qi, n.opt), -1;
      for (int i = 1; i < n.n_children; ++i)
        if (q.nodes[kids[i]].atom_pos <= q.nodes[kids[i - 1]].atom_pos) return err = mrk_fail(MRK_E_INVAL, "query %u: phrase atom positions must ascend", qi), -1;
      sph_isort(ord, key);
      IntVec nodes_q(n.n_children);
      int inner = -1;
      for (int i = 0; i < n.n_children; ++i) { // (keywords enter in chain order)
        nodes_q[ord[i]] = term_node(kids[ord[i]], n.field_mask);
        nway_step(inner, nodes_q[ord[i]], ord, i);
      }
      GenNode g{};
      g.kind = n.op == MRK_OP_PHRASE ? GN_PHRASE : GN_PROX;
      g.n_kids = 1, g.kid[0] = (uint8_t)inner, g.n_words = (uint8_t)n.n_children, g.opt = n.opt;
      for (int i = 0; i < n.n_children; ++i) g.aux[i] = G.prog.nodes[nodes_q[i]].kid[0];
      return G.add(g, G.plan[inner], INT_MAX, G.atom[nodes_q[0]]);
    }
    case MRK_OP_NEAR: { // CreateMultiNode<ExtMultinear_c>: operands of any kind; two of them on the device (see mrk_keval.h)
      // three and more operands: the folded hit's query position depends on the docs the node evaluated before (m_uFirstQpos
      // is never reset), which a probe launch reconstructs -- for a node every doc of which reaches the evaluator: the root
      if (n.n_children > 2 && (depth != 0 || n.n_children > MRK_MAX_AND_TERMS))
        return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: NEAR over %d operands below another operator (device path: two there, up to %d at the root)", qi,
                              n.n_children, MRK_MAX_AND_TERMS), -1;
      if (n.n_children > 2) T.gen_nearn = true;
      if (n.opt <= 0 || n.opt > (1 << 20)) return err = mrk_fail(MRK_E_INVAL, "query %u: NEAR distance %d", qi, n.opt), -1;
      for (int i = 0; i < n.n_children; ++i) {
        const int cop = q.nodes[kids[i]].op;
        if (cop != MRK_OP_TERM && cop != MRK_OP_PHRASE && cop != MRK_OP_PROXIMITY && cop != MRK_OP_NEAR)
          return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: NEAR over AND / OR groups (the reference's answer for them is not understood: parity unpinned)", qi), -1;
      }
      sph_isort(ord, key);
      IntVec nodes_q(n.n_children);
      int inner = -1;
      for (int i = 0; i < n.n_children; ++i) {
        const int c = build_gen(seg, q, kids[ord[i]], T, G, qi, depth + 1, err);
        if (c < 0) return -1;
        nodes_q[ord[i]] = c;
        nway_step(inner, c, ord, i);
      }
      GenNode g{};
      g.kind = GN_NEAR, g.n_kids = 1, g.kid[0] = (uint8_t)inner, g.opt = n.opt, g.n_words = (uint8_t)n.n_children;
      return G.add(g, G.plan[inner], INT_MAX, G.atom[nodes_q[0]]);
    }
    case MRK_OP_QUORUM: { // :1638-1686
      if (!all_terms || any_tp || n.n_children < 2) return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: quorum over plain keywords only", qi), -1;
      if (n.opt < 1) return err = mrk_fail(MRK_E_INVAL, "query %u: quorum threshold %d", qi, n.opt), -1;
      if (n.opt != 1 && n.opt < n.n_children) { // a real ExtQuorum_c: keywords in query-position order
        if (T.quorum || n.n_children > QUORUM_EVENTS || n.n_children > MRK_MAX_AND_TERMS)
          return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: quorum nodes on the device path: one per query, <= %d keywords", qi, QUORUM_EVENTS), -1;
        for (int i = 0; i < n.n_children; ++i) ord[i] = i;
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return q.nodes[kids[a]].atom_pos < q.nodes[kids[b]].atom_pos; });
        for (int i = 0; i < n.n_children; ++i)
          for (int j = 0; j < i; ++j)
            if (q.nodes[kids[i]].term_id >= 0 && q.nodes[kids[j]].term_id == q.nodes[kids[i]].term_id)
              return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: quorum with a repeated keyword (m_bHasDupes) is not on the device path", qi), -1;
        const uint32_t all = seg->n_fields >= 32 ? 0xFFFFFFFFu : (1u << seg->n_fields) - 1u;
        GenNode g{};
        g.kind = GN_QUORUM, g.n_kids = (uint8_t)n.n_children, g.opt = n.opt;
        const size_t nodes0 = T.nodes.size();
        T.q_kw0 = (int)T.kws.size();
        for (int i = 0; i < n.n_children; ++i) {
          int pl;
          g.kid[i] = (uint8_t)keyword(kids[ord[i]], n.field_mask, pl);
          if ((T.kws.back().queried32 & all) != all) // where a keyword's stream ends is only known for unrestricted keywords
            return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: field-limited keywords in a quorum are not on the device path", qi), -1;
        }
        T.nodes.n = (int)nodes0; // the quorum node reads its keywords' presence bits itself
        T.quorum = true;
        T.q_n = n.n_children, T.q_thr = n.opt;
        PlanNode pn;
        pn.op = PN_QUORUM;
        T.nodes.push_back(pn);
        return G.add(g, (int)T.nodes.size() - 1, INT_MAX, q.nodes[kids[ord[0]]].atom_pos);
      }
      sph_isort(ord, key); // threshold 1: an ExtOr_c chain; threshold >= words: an ExtAnd_c chain; both over the words by doc count
      int cur = term_node(kids[ord[0]], n.field_mask);
      for (int i = 1; i < n.n_children; ++i) {
        const int r = term_node(kids[ord[i]], n.field_mask);
        cur = n.opt == 1 ? twofer(GN_OR, PN_OR, cur, r) : twofer(GN_AND, PN_AND, cur, r);
      }
      return cur;
    }
    case MRK_OP_BEFORE: { // CreateOrderNode (:1044-1073): children as they come
      if (n.n_children < 2 || n.n_children > MRK_MAX_AND_TERMS) return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: BEFORE over %d nodes", qi, n.n_children), -1;
      GenNode g{};
      g.kind = GN_ORDER, g.n_kids = (uint8_t)n.n_children;
      int pl = -1;
      for (int i = 0; i < n.n_children; ++i) {
        const int c = build_gen(seg, q, kids[i], T, G, qi, depth + 1, err);
        if (c < 0) return -1;
        g.kid[i] = (uint8_t)c;
        pl = pl < 0 ? G.plan[c] : pjoin(PN_AND, pl, G.plan[c]);
      }
      return G.add(g, pl, INT_MAX, G.atom[g.kid[0]]);
    }
    case MRK_OP_AND: {
      if (all_terms && n.n_children > 1 && any_tp) { // a position modifier rules the multi-and node out (:1724-1762): an ExtAnd_c chain by doc count
        sph_isort(ord, key);
        int cur = term_node(kids[ord[0]], 0xFFFFFFFFu);
        for (int i = 1; i < n.n_children; ++i) cur = twofer(GN_AND, PN_AND, cur, term_node(kids[ord[i]], 0xFFFFFFFFu));
        return cur;
      }
      if (all_terms && n.n_children > 1) { // CreateMultiAndNode (:1118-1138) + ExtMultiAnd_T ctor (:2772-2798)
        if (n.n_children > MRK_MAX_AND_TERMS) return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: %d keywords (device path: <= %d)", qi, n.n_children, MRK_MAX_AND_TERMS), -1;
        sph_isort(ord, key);
        GenNode g{};
        g.kind = GN_MULTIAND, g.n_kids = (uint8_t)n.n_children;
        int pl = -1;
        for (int i = 0; i < n.n_children; ++i) {
          int p1;
          g.kid[i] = (uint8_t)keyword(kids[ord[i]], 0xFFFFFFFFu, p1);
          g.aux[i] = (uint8_t)ord[i];
          if (q.nodes[kids[ord[i]]].field_mask != 0xFFFFFFFFu) g.flags |= 2u;
          pl = pl < 0 ? p1 : pjoin(PN_AND, pl, p1);
        }
        return G.add(g, pl, INT_MAX, T.kws[g.kid[0]].atom_pos);
      }
      int cur = -1;
      for (int i = 0; i < n.n_children; ++i) {
        const int c = build_gen(seg, q, kids[i], T, G, qi, depth + 1, err);
        if (c < 0) return -1;
        cur = cur < 0 ? c : twofer(GN_AND, PN_AND, cur, c);
      }
      return cur;
    }
    case MRK_OP_SENTENCE:
    case MRK_OP_PARAGRAPH: { // generic create (:1785-1803): pCur = new ExtUnit_c ( pCur, pNext, fields, setup, MAGIC_WORD_... )
      int cur = -1;
      for (int i = 0; i < n.n_children; ++i) {
        const int c = build_gen(seg, q, kids[i], T, G, qi, depth + 1, err);
        if (c < 0) return -1;
        cur = cur < 0 ? c : twofer(GN_UNIT, PN_AND, cur, c);
        if (G.prog.nodes[cur].kind == GN_UNIT && cur != c) G.prog.nodes[cur].aux[0] = 0xFF;
      }
      if (n.term_id >= 0 && (uint32_t)n.term_id < seg->terms.size() && seg->terms[n.term_id].docs) {
        // the boundary keyword: one slot, located for every candidate (MAYBE: a doc without boundaries is a plain AND)
        PlanKw k{};
        k.term_id = n.term_id, k.node = ni, k.docs = (int)seg->terms[n.term_id].docs, k.boost = 1.0f, k.queried32 = n.field_mask, k.hidden = true;
        T.kws.push_back(k);
        PlanNode pn;
        pn.op = PN_TERM;
        pn.kw = (int)T.kws.size() - 1;
        T.nodes.push_back(pn);
        const int dot_plan = (int)T.nodes.size() - 1;
        for (uint32_t g = 0; g < G.prog.n_nodes; ++g)
          if (G.prog.nodes[g].kind == GN_UNIT && G.prog.nodes[g].aux[0] == 0xFF && G.prog.nodes[g].aux[1] == 0) G.prog.nodes[g].aux[0] = (uint8_t)pn.kw, G.prog.nodes[g].aux[1] = 1;
        G.plan[cur] = pjoin(PN_MAYBE, G.plan[cur], dot_plan);
      } else
        for (uint32_t g = 0; g < G.prog.n_nodes; ++g)
          if (G.prog.nodes[g].kind == GN_UNIT && G.prog.nodes[g].aux[0] == 0xFF) G.prog.nodes[g].aux[1] = 1; // (settled: no boundary keyword)
      return cur;
    }
    case MRK_OP_OR:
    case MRK_OP_MAYBE:
    case MRK_OP_ANDNOT:
    case MRK_OP_NOTNEAR: {
      if (n.op == MRK_OP_NOTNEAR && (n.opt <= 0 || n.opt > (1 << 20))) return err = mrk_fail(MRK_E_INVAL, "query %u: NOTNEAR distance %d", qi, n.opt), -1;
      int cur = -1;
      for (int i = 0; i < n.n_children; ++i) {
        const int c = build_gen(seg, q, kids[i], T, G, qi, depth + 1, err);
        if (c < 0) return -1;
        if (cur < 0)
          cur = c;
        else if (n.op == MRK_OP_OR)
          cur = twofer(GN_OR, PN_OR, cur, c);
        else if (n.op == MRK_OP_MAYBE)
          cur = twofer(GN_MAYBE, PN_MAYBE, cur, c);
        else // whether the right side holds the doc is only known after its hits were read: the left side carries the candidates
          cur = twofer(n.op == MRK_OP_ANDNOT ? GN_ANDNOT : GN_NOTNEAR, PN_MAYBE, cur, c, n.opt);
      }
      return cur;
    }
    default: return err = mrk_fail(MRK_E_UNSUPPORTED, "query %u: operator %d not on the device path yet", qi, n.op), -1;
  }
}

// keywords whose doc streams together contain every possible match of the subtree
static void cover_of(const PlanTree& T, int ni, IntVec& out) {
  const PlanNode& n = T.nodes[ni];
  if (n.op == PN_QUORUM) { // a match holds >= thr of the n keywords, hence at least one of ANY n - thr + 1: the cheapest ones
    IntVec k;
    for (int i = 0; i < T.q_n; ++i) k.push_back(T.q_kw0 + i);
    std::stable_sort(k.begin(), k.end(), [&](int a, int b) { return T.kws[a].docs < T.kws[b].docs; });
    for (int i = 0; i < T.q_n - T.q_thr + 1; ++i)
      if (T.kws[k[i]].docs > 0) out.push_back(k[i]); // a keyword without postings drives nothing
    return;
  }
  if (n.op == PN_TERM) {
    out.push_back(n.kw);
    return;
  }
  if (n.op == PN_OR) {
    cover_of(T, n.l, out);
    cover_of(T, n.r, out);
    return;
  }
  if (n.op == PN_AND) {
    IntVec a, b;
    cover_of(T, n.l, a);
    cover_of(T, n.r, b);
    uint64_t ca = 0, cb = 0;
    for (int k : a) ca += (uint64_t)T.kws[k].docs;
    for (int k : b) cb += (uint64_t)T.kws[k].docs;
    const IntVec& w = (cb < ca || (cb == ca && b.size() < a.size())) ? b : a;
    out.append(w.begin(), w.end());
    return;
  }
  cover_of(T, n.l, out); // MAYBE, ANDNOT, PHRASEFIX: the left side carries the docs
}

// keywords that must be present for the subtree to match
static uint32_t required_of(const PlanTree& T, int ni) {
  const PlanNode& n = T.nodes[ni];
  if (n.op == PN_QUORUM) return 0; // no single keyword is needed
  if (n.op == PN_TERM) return 1u << n.kw;
  if (n.op == PN_AND) return required_of(T, n.l) | required_of(T, n.r);
  if (n.op == PN_OR) return required_of(T, n.l) & required_of(T, n.r);
  return required_of(T, n.l);
}

static void fill_term(const mrk_segment* seg, const PlanKw& k, DevTerm& dt) {
  memset(&dt, 0, sizeof dt);
  dt.queried32 = k.queried32;
  dt.idf = k.weighted_first ? k.idf : 0.0f;
  dt.qpos = (uint32_t)k.atom_pos;
  dt.tp_kind = (uint32_t)k.tp_kind;
  dt.tp_max = (uint32_t)k.tp_max;
  if (!k.docs) return; // keyword without postings: nblocks = 0, never present
  const HostTerm& h = seg->terms[k.term_id];
  dt.blk_first = h.blk_first;
  dt.nblocks = h.nblocks;
  dt.docs = h.docs;
  dt.spd_end = h.doclist_off + h.doclist_len;
  dt.exc_first = h.exc_first;
  dt.exc_n = h.exc_n;
  dt.bm_off = h.bm_off;
  dt.dir_off = h.dir_off;
}

// the weight-range estimates below only shape the pruning bins: with absurd field weights they saturate instead of overflowing
static int64_t sat_mul(int64_t a, int64_t b) {
  const __int128 v = (__int128)a * b, lim = (__int128)1 << 61;
  return (int64_t)(v > lim ? lim : v < -lim ? -lim : v);
}
static int64_t sat_add(int64_t a, int64_t b) {
  const __int128 v = (__int128)a + b, lim = (__int128)1 << 61;
  return (int64_t)(v > lim ? lim : v < -lim ? -lim : v);
}

void mrk::weight_sum_range(const int32_t* weights, uint32_t nwf, int64_t& rmin, int64_t& rmax) {
  rmin = INT64_MAX, rmax = INT64_MIN;
  if (nwf <= 8) {
    for (uint32_t m = 0; m < (1u << nwf); ++m) { // (every mask of the segment's fields; bits beyond them change nothing)
      int64_t r = 0;
      if (!m)
        r = 1;
      else
        for (uint32_t f = 0; f < nwf; ++f)
          if (m & (1u << f)) r += weights[f];
      rmin = std::min(rmin, r);
      rmax = std::max(rmax, r);
    }
    return;
  }
  // 2^nwf masks are too many to walk: the least non-empty sum takes every negative weight (or, with none, the smallest single
  // weight), the largest every positive one (or, with none, the largest single weight); the empty mask weighs 1
  int64_t neg = 0, pos = 0, wmin = INT64_MAX, wmax = INT64_MIN;
  bool any_neg = false, any_pos = false;
  for (uint32_t f = 0; f < nwf && f < 32; ++f) {
    const int64_t w = weights[f];
    if (w < 0) neg += w, any_neg = true;
    if (w > 0) pos += w, any_pos = true;
    wmin = std::min(wmin, w);
    wmax = std::max(wmax, w);
  }
  rmin = std::min<int64_t>(1, any_neg ? neg : wmin);
  rmax = std::max<int64_t>(1, any_pos ? pos : wmax);
}

// The range of a column's mapped keys in the DESCENDING order, once per (segment, locator, kind): the pruning bins' geometry.
// Answers the entry's place in seg->sort_ranges (a later call may move the entries: take pointers once every column was looked up)
static size_t column_range(const mrk_segment* seg, int32_t bit_offset, int32_t bit_count, int32_t kind) {
  for (size_t i = 0; i < seg->sort_ranges.size(); ++i) {
    const mrk_segment::SortRange& r = seg->sort_ranges[i];
    if (r.bit_offset == bit_offset && r.bit_count == bit_count && r.is_float == kind) return i;
  }
  mrk_segment::SortRange r{bit_offset, bit_count, kind, 0xFFFFFFFFu, 0u, false};
  const uint32_t stride = seg->dev.attr_stride, item = (uint32_t)bit_offset >> 5, shift = (uint32_t)bit_offset & 31u;
  const uint32_t fl = SORT_DESC | (kind == MRK_SORTKEY_FLOAT ? SORT_FLOAT : 0u);
  const uint64_t rows = seg->h_attrs.size() / stride;
  if (kind == MRK_SORTKEY_INT64) {
    r.lo64 = ~0ull, r.hi64 = 0;
    for (uint64_t i = 0; i < rows; ++i) {
      const uint64_t m = order_map_i64((int64_t)(((uint64_t)seg->h_attrs[i * stride + item + 1] << 32) | seg->h_attrs[i * stride + item]), true);
      r.lo64 = std::min(r.lo64, m), r.hi64 = std::max(r.hi64, m);
    }
  } else
    for (uint64_t i = 0; i < rows; ++i) {
      const uint32_t v = sort_extract(seg->h_attrs[i * stride + item], shift, (uint32_t)bit_count);
      if (kind == MRK_SORTKEY_FLOAT && sort_is_nan(v)) r.has_nan = true;
      const uint32_t m = sort_map_key(v, fl);
      r.lo = std::min(r.lo, m), r.hi = std::max(r.hi, m);
    }
  seg->sort_ranges.push_back(r);
  return seg->sort_ranges.size() - 1;
}

// ---- plan_query's stages: member functions of one PlanState per query, called top to bottom by plan_query.  A stage that can
// decline the query answers MRK_OK or the code (message set).

// The sorter's order as the stages after resolve_order / resolve_sort read it, whether it came as mrk_query.sort or mrk_query.order:
// no part = relevance; one part of <= 32 bits = the narrow key (DevQuery::sort_on 1); a 64-bit key (one INT64 part, or two parts) = wide
struct KeyPart {
  int32_t kind, bit_offset, bit_count;
  bool desc;
  const mrk_segment::SortRange* range; // the column's mapped keys (DESCENDING order)
  uint32_t flags() const { return (kind == MRK_SORTKEY_FLOAT ? SORT_FLOAT : 0u) | (desc ? SORT_DESC : 0u); }
  uint32_t item() const { return (uint32_t)bit_offset >> 5; }
};
struct KeySpec {
  int n_parts = 0;
  KeyPart part[MRK_MAX_ORDER_PARTS];
  int32_t tie = 0; // mrk_sort::then_weight
  bool wide = false;
  int32_t wfirst = 0; // mrk_order::then_weight = MRK_ORDER_WEIGHT_FIRST_*: the weight leads (1 DESC / 2 ASC), n_parts may be 0
  bool sorted() const { return n_parts > 0 || wfirst != 0; }
};

struct PlanState {
  // what plan_query was handed
  const mrk_segment* const seg;
  const mrk_query& q;
  const bool use_packed;
  const uint32_t qi;
  const mrk_group* const group; // mrk_batch_submit_grouped's spec for this query, or NULL
  const mrk_aggrs* const aggrs; // mrk_batch_submit_aggr's aggregates for this (grouped) query, or NULL
  const mrk_group_mva* const mva; // mrk_batch_submit_mva's multi-value group attribute for this (grouped) query, or NULL
  // what the stages work out, in their order
  KeySpec order;
  bool filtered = false; // the query reads attribute rows: the packed block scan's EXT instances only
  PlanTree T;
  std::optional<GenBuild> gen_build; // (built only for the shapes that go to the generic evaluator: 0.8 KB to clear)
  int root = -1, n = 0; // the tree's root node, its keywords
  uint32_t ranker = 0;
  bool single_word = false, pure_and = false, prox = false;
  IntVec words; // distinct words in GetQwords traversal order
  bool got_dupes = false;
  IntVec cover; // driver keywords: one pass each
  uint32_t req = 0;
  bool empty = false;
  uint64_t bytes = 0, pbytes = 0;

  // a key of <= 32 bits: 1..32 bits inside one dword, a float takes all 32.  `noun` / `key` name the spec in the messages
  static int check_key_locator(uint32_t qi, const char* noun, const char* key, int32_t kind, int32_t bit_offset, int32_t bit_count) {
    if (bit_count < 1 || bit_count > 32 || (bit_offset & 31) + bit_count > 32)
      return mrk_fail(MRK_E_INVAL, "query %u: %s locator %d/%d is not 1..32 bits inside one dword", qi, noun, bit_offset, bit_count);
    if (kind == MRK_SORTKEY_FLOAT && bit_count != 32) return mrk_fail(MRK_E_INVAL, "query %u: a float %s needs a 32-bit attribute", qi, key);
    return MRK_OK;
  }
  static int check_key_in_row(const mrk_segment* seg, uint32_t qi, const char* noun, int32_t bit_offset, int32_t bit_count) {
    if ((uint64_t)bit_offset + (uint64_t)bit_count > (uint64_t)seg->dev.attr_stride * 32)
      return mrk_fail(MRK_E_INVAL, "query %u: %s locator %d/%d outside the %u-dword row", qi, noun, bit_offset, bit_count, seg->dev.attr_stride);
    return MRK_OK;
  }

  // mrk_query.order: validated before anything is read.  One part of <= 32 bits IS mrk_query.sort's order and is planned as that (the
  // same passes, items and bins; resolve_sort finishes it); a 64-bit key (INT64, two parts) is resolved here, its columns' ranges included.
  int resolve_order() {
    if (!q.order) return MRK_OK;
    const mrk_order& O = *q.order;
    if (q.sort) return mrk_fail(MRK_E_INVAL, "query %u: mrk_query.sort and mrk_query.order are both set", qi);
    // then_weight says where the weight stands: behind the parts (0 / 1 / 2) or, MRK_ORDER_WEIGHT_FIRST_DESC / _ASC, in front of them
    const int32_t wfirst = (O.then_weight == MRK_ORDER_WEIGHT_FIRST_DESC || O.then_weight == MRK_ORDER_WEIGHT_FIRST_ASC) ? O.then_weight & 3 : 0;
    if ((O.n_parts < 1 && !(wfirst == 2 && O.n_parts == 0)) || O.n_parts > MRK_MAX_ORDER_PARTS)
      return mrk_fail(MRK_E_INVAL, "query %u: order of %d parts (1..%d)", qi, O.n_parts, MRK_MAX_ORDER_PARTS);
    if (!wfirst && (O.then_weight < 0 || O.then_weight > 2)) return mrk_fail(MRK_E_INVAL, "query %u: order tie rule %d", qi, O.then_weight);
    for (int p = 0; p < O.n_parts; ++p) {
      const mrk_order_part& P = O.parts[p];
      if (P.kind != MRK_SORTKEY_INT && P.kind != MRK_SORTKEY_FLOAT && P.kind != MRK_SORTKEY_INT64) return mrk_fail(MRK_E_INVAL, "query %u: order part %d: key kind %d", qi, p, P.kind);
      if (P.kind == MRK_SORTKEY_INT64 && O.n_parts != 1) return mrk_fail(MRK_E_INVAL, "query %u: a 64-bit order part stands alone (part %d of %d)", qi, p, O.n_parts);
      if (P.bit_offset < 0) continue; // (a blob-stored part: declined below, once every part's shape has been checked)
      if (P.kind == MRK_SORTKEY_INT64) {
        if (P.bit_count != 64 || (P.bit_offset & 31) != 0) return mrk_fail(MRK_E_INVAL, "query %u: order locator %d/%d is not 64 dword-aligned bits", qi, P.bit_offset, P.bit_count);
      } else if (int rc = check_key_locator(qi, "order", "order part", P.kind, P.bit_offset, P.bit_count))
        return rc;
      if (seg->dev.attrs && seg->dev.attr_stride)
        if (int rc = check_key_in_row(seg, qi, "order", P.bit_offset, P.bit_count)) return rc;
    }
    order.n_parts = O.n_parts;
    order.tie = wfirst ? 0 : O.then_weight;
    order.wfirst = wfirst;
    for (int p = 0; p < O.n_parts; ++p) order.part[p] = KeyPart{O.parts[p].kind, O.parts[p].bit_offset, O.parts[p].bit_count, O.parts[p].desc != 0, nullptr};
    // (a weight-first order is resolved here whatever its parts: one candidate layout for all of them, none of it mrk_query.sort's)
    if (O.n_parts == 1 && O.parts[0].kind != MRK_SORTKEY_INT64 && !wfirst) return MRK_OK; // (resolve_sort checks it as the mrk_sort it is)
    order.wide = O.n_parts == 2 || (O.n_parts == 1 && O.parts[0].kind == MRK_SORTKEY_INT64);
    for (int p = 0; p < O.n_parts; ++p)
      if (O.parts[p].bit_offset < 0) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: order by a blob-stored or computed attribute (part %d has no row locator)", qi, p);
    if (O.n_parts && (!seg->dev.attrs || seg->h_attrs.empty()))
      return mrk_fail(MRK_E_UNSUPPORTED, "query %u: ordering by attributes needs the segment's attribute rows (mrk_segment_set_attrs)", qi);
    if (!use_packed) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: ordered queries run on the packed path only", qi);
    if (q.cutoff > 0) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: cutoff next to an order (which rows count depends on the scan order)", qi);
    size_t at[MRK_MAX_ORDER_PARTS];
    for (int p = 0; p < O.n_parts; ++p) {
      at[p] = column_range(seg, O.parts[p].bit_offset, O.parts[p].bit_count, O.parts[p].kind);
      if (seg->sort_ranges[at[p]].has_nan) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: the float column of order part %d holds a NaN (no strict weak order)", qi, p);
    }
    for (int p = 0; p < O.n_parts; ++p) order.part[p].range = &seg->sort_ranges[at[p]];
    return MRK_OK;
  }

  // The narrow key: mrk_query.sort, or the mrk_query.order that is one.  Checked before anything is read: a hostile locator ends here.
  int resolve_sort() {
    if (q.sort) {
      const mrk_sort& Q = *q.sort;
      order.n_parts = 1;
      order.tie = Q.then_weight;
      order.part[0] = KeyPart{Q.kind, Q.bit_offset, Q.bit_count, Q.desc != 0, nullptr};
    } else if (order.n_parts != 1 || order.wide || order.wfirst)
      return MRK_OK;
    KeyPart& P = order.part[0];
    if (P.kind != MRK_SORTKEY_INT && P.kind != MRK_SORTKEY_FLOAT) return mrk_fail(MRK_E_INVAL, "query %u: sort key kind %d", qi, P.kind);
    if (order.tie < 0 || order.tie > 2) return mrk_fail(MRK_E_INVAL, "query %u: sort tie rule %d", qi, order.tie);
    if (P.bit_offset < 0) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: sort by a blob-stored or computed attribute (no row locator)", qi);
    if (P.bit_count == 64 && (P.bit_offset & 31) == 0 && seg->dev.attrs && (uint64_t)P.bit_offset + 64 <= (uint64_t)seg->dev.attr_stride * 32)
      return mrk_fail(MRK_E_UNSUPPORTED, "query %u: sort by a 64-bit attribute (device path: <= 32 bits)", qi);
    if (int rc = check_key_locator(qi, "sort", "sort key", P.kind, P.bit_offset, P.bit_count)) return rc;
    if (!seg->dev.attrs || seg->h_attrs.empty())
      return mrk_fail(MRK_E_UNSUPPORTED, "query %u: sorting by an attribute needs the segment's attribute rows (mrk_segment_set_attrs)", qi);
    if (int rc = check_key_in_row(seg, qi, "sort", P.bit_offset, P.bit_count)) return rc;
    if (!use_packed) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: sorted queries run on the packed path only", qi);
    if (q.cutoff > 0) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: cutoff next to a sort (which rows count depends on the scan order)", qi);
    // the column's range of mapped keys: the pruning bins' geometry; a NaN ends the query here
    P.range = &seg->sort_ranges[column_range(seg, P.bit_offset, P.bit_count, P.kind)];
    if (P.range->has_nan) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: the float sort column holds a NaN (no strict weak order)", qi);
    return MRK_OK;
  }

  // mrk_group: validated exactly as the sort's locator is, before anything is read; what declines a sort declines a group
  int resolve_group() const {
    if (!group) return MRK_OK;
    const mrk_group& G = *group;
    if (G.sort_by != MRK_GROUPSORT_KEY && G.sort_by != MRK_GROUPSORT_COUNT && G.sort_by != MRK_GROUPSORT_WEIGHT)
      return mrk_fail(MRK_E_INVAL, "query %u: group sort_by %d", qi, G.sort_by);
    if (G.desc != 0 && G.desc != 1) return mrk_fail(MRK_E_INVAL, "query %u: group desc %d (0 or 1)", qi, G.desc);
    if (mva) return resolve_group_mva();
    if (G.bit_offset < 0) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: group by a blob-stored or computed attribute (no row locator)", qi);
    if (G.bit_count == 64 && (G.bit_offset & 31) == 0 && seg->dev.attrs && (uint64_t)G.bit_offset + 64 <= (uint64_t)seg->dev.attr_stride * 32)
      return mrk_fail(MRK_E_UNSUPPORTED, "query %u: group by a 64-bit attribute (device path: <= 32 bits)", qi);
    if (int rc = check_key_locator(qi, "group", "group key", MRK_SORTKEY_INT, G.bit_offset, G.bit_count)) return rc;
    if (seg->dev.attrs && seg->dev.attr_stride)
      if (int rc = check_key_in_row(seg, qi, "group", G.bit_offset, G.bit_count)) return rc;
    if (q.sort || q.order) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: a group next to mrk_query.sort / mrk_query.order (the within-group order is relevance)", qi);
    if (!seg->dev.attrs || seg->h_attrs.empty())
      return mrk_fail(MRK_E_UNSUPPORTED, "query %u: grouping by an attribute needs the segment's attribute rows (mrk_segment_set_attrs)", qi);
    if (!use_packed) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: grouped queries run on the packed path only", qi);
    if (q.cutoff > 0) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: cutoff next to a group (which rows count depends on the scan order)", qi);
    return MRK_OK;
  }
  // mrk_group_mva: the group's attribute is a multi-value attribute in the blob pool; mrk_group's locator is ignored, its order was
  // checked above.  The tests and the wording of an MVA filter (translate_filter), then what the device declines, then what declines
  // every group
  int resolve_group_mva() const {
    const mrk_group_mva& M = *mva;
    if (M.mva_bits != 32 && M.mva_bits != 64) return mrk_fail(MRK_E_INVAL, "query %u: MVA width %d", qi, M.mva_bits);
    if (M.n_blob_attrs < 1 || M.n_blob_attrs > 255 || M.blob_attr_id < 0 || M.blob_attr_id >= M.n_blob_attrs)
      return mrk_fail(MRK_E_INVAL, "query %u: blob attribute %d of %d (the segment's rows hold %u)", qi, M.blob_attr_id, M.n_blob_attrs, seg->n_blob_attrs);
    if (!seg->dev.blobs) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: grouping by an MVA needs the segment's blob pool (mrk_segment_set_blobs)", qi);
    if ((uint32_t)M.n_blob_attrs != seg->n_blob_attrs)
      return mrk_fail(MRK_E_INVAL, "query %u: blob attribute %d of %d (the segment's rows hold %u)", qi, M.blob_attr_id, M.n_blob_attrs, seg->n_blob_attrs);
    if (seg->dev.attr_stride < 4) return mrk_fail(MRK_E_INVAL, "query %u: rows of %u dwords hold no blob locator", qi, seg->dev.attr_stride);
    if (M.mva_bits == 64) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: group by a 64-bit MVA (device path: the group key has 32 bits)", qi);
    if (aggrs) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: aggregates next to a group by an MVA (one accumulator slot per match, not per pushed value)", qi);
    if (q.sort || q.order) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: a group next to mrk_query.sort / mrk_query.order (the within-group order is relevance)", qi);
    if (!seg->dev.attrs || seg->h_attrs.empty())
      return mrk_fail(MRK_E_UNSUPPORTED, "query %u: grouping by an attribute needs the segment's attribute rows (mrk_segment_set_attrs)", qi);
    if (!use_packed) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: grouped queries run on the packed path only", qi);
    if (q.cutoff > 0) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: cutoff next to a group (which rows count depends on the scan order)", qi);
    return MRK_OK;
  }
  // mrk_aggrs: the aggregate stage, next to the group's.  check_aggrs, in front of resolve_group: everything hostile is MRK_E_INVAL
  // before a row is read, whatever the group turns out to be.  decline_aggrs, behind it: what the device declines, each message naming
  // the aggregate it declines
  int check_aggrs() const {
    if (!aggrs) return MRK_OK;
    const mrk_aggrs& A = *aggrs;
    if (!group) return mrk_fail(MRK_E_INVAL, "query %u: aggregates without a group", qi);
    if (A.n < 1 || A.n > MRK_MAX_AGGRS) return mrk_fail(MRK_E_INVAL, "query %u: %d aggregates (1..%d)", qi, A.n, MRK_MAX_AGGRS);
    if (A.order_by < -1 || A.order_by >= A.n) return mrk_fail(MRK_E_INVAL, "query %u: aggregate order_by %d of %d aggregates", qi, A.order_by, A.n);
    if (A.order_by >= 0 && group->sort_by != MRK_GROUPSORT_KEY)
      return mrk_fail(MRK_E_INVAL, "query %u: aggregate order_by %d next to group sort_by %d (MRK_GROUPSORT_KEY with an aggregate order)", qi, A.order_by, group->sort_by);
    for (int i = 0; i < A.n; ++i) {
      const mrk_aggr& G = A.a[i];
      if (G.func != MRK_AGGR_SUM && G.func != MRK_AGGR_MIN && G.func != MRK_AGGR_MAX) return mrk_fail(MRK_E_INVAL, "query %u: aggregate %d: function %d", qi, i, G.func);
      if (G.kind != MRK_SORTKEY_INT && G.kind != MRK_SORTKEY_FLOAT && G.kind != MRK_SORTKEY_INT64) return mrk_fail(MRK_E_INVAL, "query %u: aggregate %d: source kind %d", qi, i, G.kind);
      if (G.flags & ~MRK_AGGR_WIDEN) return mrk_fail(MRK_E_INVAL, "query %u: aggregate %d: flags 0x%x", qi, i, (unsigned)G.flags);
      if ((G.flags & MRK_AGGR_WIDEN) && G.kind != MRK_SORTKEY_INT) return mrk_fail(MRK_E_INVAL, "query %u: aggregate %d: MRK_AGGR_WIDEN on a source of kind %d (an INT source only)", qi, i, G.kind);
      if (G.bit_offset < 0) continue; // (a blob-stored source: declined below, once every aggregate's shape has been checked)
      if (G.kind == MRK_SORTKEY_INT64) {
        if (G.bit_count != 64 || (G.bit_offset & 31) != 0) return mrk_fail(MRK_E_INVAL, "query %u: aggregate %d: locator %d/%d is not 64 dword-aligned bits", qi, i, G.bit_offset, G.bit_count);
      } else if (int rc = check_key_locator(qi, "aggregate", "aggregate source", G.kind, G.bit_offset, G.bit_count))
        return rc;
      if (seg->dev.attrs && seg->dev.attr_stride)
        if (int rc = check_key_in_row(seg, qi, "aggregate", G.bit_offset, G.bit_count)) return rc;
    }
    return MRK_OK;
  }
  int decline_aggrs() const {
    if (!aggrs) return MRK_OK;
    const mrk_aggrs& A = *aggrs;
    static const char* const fn[] = {"", "SUM", "MIN", "MAX"};
    for (int i = 0; i < A.n; ++i) {
      const mrk_aggr& G = A.a[i];
      if (G.kind == MRK_SORTKEY_FLOAT)
        return mrk_fail(MRK_E_UNSUPPORTED, "query %u: aggregate %d: %s of a float attribute (a float SUM depends on the arrival order, float MIN / MAX at NaN and +-0)", qi, i, fn[G.func]);
      if (G.bit_offset < 0) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: aggregate %d: %s of a blob-stored or computed attribute (no row locator)", qi, i, fn[G.func]);
    }
    if (A.order_by >= 0 && (A.a[A.order_by].kind == MRK_SORTKEY_INT64 || (A.a[A.order_by].flags & MRK_AGGR_WIDEN)))
      return mrk_fail(MRK_E_UNSUPPORTED, "query %u: groups ordered by aggregate %d, %s with a 64-bit result (device path: a 32-bit aggregate orders)", qi, A.order_by, fn[A.a[A.order_by].func]);
    return MRK_OK;
  }

  // ... and its words of the descriptor: where the key lies in the row, the groups' order, the query's table in the batch's arena.
  // A grouped query publishes no candidates and needs no pruning threshold
  void reserve_group(DevQuery& dq, BatchPlan& plan) const {
    const mrk_group& G = *group;
    dq.cand_cap = dq.sort_cap = 0;
    dq.grp_on = 1;
    dq.grp_item = (uint32_t)G.bit_offset >> 5, dq.grp_shift = (uint32_t)G.bit_offset & 31u, dq.grp_bits = (uint32_t)G.bit_count;
    if (mva) // the values come from the blob pool at the flush: the scan's read of the group dword reads the row's first, and is ignored
      dq.grp_item = 0, dq.grp_shift = 0, dq.grp_bits = 32, dq.grp_pad = group_mva_word((uint32_t)mva->mva_bits, (uint32_t)mva->blob_attr_id, (uint32_t)mva->n_blob_attrs);
    dq.grp_sort_by = (uint32_t)G.sort_by, dq.grp_desc = (uint32_t)G.desc;
    dq.grp_slots = group_slots_for((uint32_t)q.max_matches);
    dq.grp_off = plan.group_total;
    if (aggrs) { // one accumulator plane per aggregate behind the counts (mrk_kgroup.h)
      dq.grp_naggr = (uint32_t)aggrs->n, dq.grp_order_aggr = (uint32_t)(aggrs->order_by + 1);
      for (int i = 0; i < aggrs->n; ++i) {
        const mrk_aggr& A = aggrs->a[i];
        const bool src64 = A.kind == MRK_SORTKEY_INT64;
        dq.grp_aggr_item[i] = (uint32_t)A.bit_offset >> 5;
        dq.grp_aggr_op[i] = aggr_op_word((uint32_t)A.func, (uint32_t)A.bit_offset & 31u, src64 ? 0u : (uint32_t)A.bit_count, src64, (A.flags & MRK_AGGR_WIDEN) != 0);
      }
    }
    plan.group_total += group_table_words(dq.grp_slots, dq.grp_naggr);
  }

  // what plan_query checks of the query itself before the tree is walked
  int check_query() const {
    if (!q.nodes || q.n_nodes <= 0 || q.root < 0 || q.root >= q.n_nodes) return mrk_fail(MRK_E_INVAL, "query %u: bad tree", qi);
    for (int i = 0; i < q.n_nodes; ++i) // (ExtHit_t::m_uQuerypos is a WORD, sphinxint.h:733; the arithmetic on positions below assumes as much)
      if (q.nodes[i].op == MRK_OP_TERM && (q.nodes[i].atom_pos < 0 || q.nodes[i].atom_pos > 0xFFFF))
        return mrk_fail(MRK_E_INVAL, "query %u: query position %d of node %d", qi, q.nodes[i].atom_pos, i);
    if (q.max_matches <= 0 || q.max_matches > MRK_MAX_K)
      return mrk_fail(MRK_E_UNSUPPORTED, "query %u: max_matches %d outside 1..%d", qi, q.max_matches, MRK_MAX_K);
    // cutoff (MatchExtended, sphinx.cpp:12197-12199, 12261-12267): the sorter's Push() never says no (sphinxsort.cpp:722-759), so the
    // scan stops after the first `cutoff` rows that got as far as the sorter -- the caller found the last of them with a probe
    // launch (cutoff_probe, mrk_host.cpp) and hands it down as rowid_max: rows past it never reach the ranker
    if (q.cutoff > 0 && !use_packed) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: cutoff runs on the packed path only", qi);
    if (q.cutoff > MRK_MAX_K) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: cutoff %d (device path: <= %d)", qi, q.cutoff, MRK_MAX_K);
    if (q.cutoff > 0 && q.n_weight_filters > 0)
      return mrk_fail(MRK_E_UNSUPPORTED, "query %u: cutoff next to a weight filter (which rows count depends on their weights)", qi);
    return MRK_OK;
  }

  // values on the tree program's register stack at its deepest
  static int stack_depth(const PlanTree& T) {
    int sp = 0, deep = 0;
    for (const PlanNode& pn : T.nodes) {
      sp += (pn.op == PN_TERM || pn.op == PN_QUORUM) ? 1 : (pn.op == PN_PHRASEFIX || pn.op == PN_ORDERFIX) ? 0 : -1;
      deep = std::max(deep, sp);
    }
    return deep;
  }

  // What reads hit streams runs on the packed path of a segment with hit references (`what`: "NOTNEAR runs" ...) and packs a rowid
  // into 31 bits (`path`: the kernel family the message names)
  int needs_hit_refs(const char* what) const {
    if (!use_packed || !seg->dev.pk_hit) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: %s on the packed path only", qi, what);
    return MRK_OK;
  }
  int needs_rowids_31(const char* path) const {
    if (seg->total_docs >= (1ull << 31)) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: %s path needs < 2^31 docs per segment", qi, path);
    return MRK_OK;
  }

  // The evaluation tree, what it needs of the segment, the ranker: for the specialised paths (gen = false) or the generic evaluator
  int shape(bool gen) {
    if (gen) T = PlanTree(); // (the generic evaluator's turn comes second: the specialised paths found it fresh)
    int tree_err = MRK_OK;
    if (gen) {
      GenBuild& G = gen_build.emplace();
      root = build_gen(seg, q, q.root, T, G, qi, 0, tree_err);
      if (root >= 0 && G.overflow) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: tree too large for the device path", qi);
      if (root >= 0) {
        T.gen = T.force_tree = true;
        root = G.plan[root];
      }
    } else
      root = build_tree(seg, q, q.root, T, qi, 0, true, tree_err);
    if (root < 0) return tree_err;
    if (T.kws.overflow || T.nodes.overflow || T.atoms.overflow)
      return mrk_fail(MRK_E_UNSUPPORTED, "query %u: tree too large for the device path", qi);
    n = (int)T.kws.size();
    if (n > MRK_MAX_AND_TERMS) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: %d keywords (device path: <= %d)", qi, n, MRK_MAX_AND_TERMS);
    if (T.nodes.size() > 16) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: tree too large for the device path", qi);
    single_word = T.nodes.size() == 1 && T.nodes[0].op == PN_TERM; // XQQuery_t::m_bSingleWord
    pure_and = !T.force_tree; // single keyword or one ExtMultiAnd_T: the kernel's N-way AND loop, no program
    for (const PlanNode& pn : T.nodes) pure_and &= pn.op == PN_TERM || pn.op == PN_AND;
    if (pure_and && (q.nodes[q.root].op == MRK_OP_AND || q.nodes[q.root].op == MRK_OP_PHRASE || q.nodes[q.root].op == MRK_OP_PROXIMITY || q.nodes[q.root].op == MRK_OP_NEAR))
      for (int i = 0; i < q.nodes[q.root].n_children; ++i) pure_and &= q.nodes[q.children[q.nodes[q.root].first_child + i]].op == MRK_OP_TERM;
    if (!pure_and && !use_packed) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: boolean trees run on the packed path only", qi);
    // the device evaluates the program on a TREE_STACK-deep register stack
    if (!pure_and && stack_depth(T) > TREE_STACK) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: tree nests deeper than the device path evaluates", qi);

    prox = false; // a state ranker reads the hit streams
    if (gen && T.gen_nearn) {
      int mq = 0;
      for (const PlanKw& k : T.kws) mq = std::max(mq, k.atom_pos);
      if (filtered || q.cutoff > 0 || seg->dev.dead || mq >= 64)
        return mrk_fail(MRK_E_UNSUPPORTED, "query %u: NEAR over 3+ operands next to filters / cutoff / dead rows / query positions past 63 (every doc of the node must reach the evaluator)", qi);
    }
    if (gen && single_word) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: a single keyword is not a case for the generic evaluator", qi);
    if (gen) {
      if (!use_packed || !seg->dev.pk_hit || seg->total_docs >= (1ull << 31)) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: the generic evaluator runs on the packed path, < 2^31 docs per segment", qi);
    } else if (T.quorum && !T.quorum_root && q.ranker != MRK_RANK_NONE && q.ranker != MRK_RANK_BM25)
      return mrk_fail(MRK_E_UNSUPPORTED, "query %u: a quorum below another operator with a hit ranker is not on the device path", qi);
    if (T.ph_leaf && n > MAX_PROX_TERMS)
      return mrk_fail(MRK_E_UNSUPPORTED, "query %u: PHRASE in a tree of %d keywords (device path: <= %d)", qi, n, MAX_PROX_TERMS);
    if (T.notnear) { // decided over the two keywords' hits: the hit-reading kernel, <= 4 hit streams
      if (int rc = needs_hit_refs("NOTNEAR runs")) return rc;
      if (n > MAX_PROX_TERMS) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: NOTNEAR in a query of %d keywords (device path: <= %d)", qi, n, MAX_PROX_TERMS);
      if (T.termpos || T.quorum) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: NOTNEAR next to position modifiers / a quorum node", qi);
      if (int rc = needs_rowids_31("hit")) return rc;
    }
    if (T.termpos) { // whether a keyword holds a doc is decided over its hits: the hit-reading kernel, <= 4 hit streams
      if (int rc = needs_hit_refs("position modifiers run")) return rc;
      if (n > MAX_PROX_TERMS) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: position modifiers in a query of %d keywords (device path: <= %d)", qi, n, MAX_PROX_TERMS);
      if (int rc = needs_rowids_31("hit")) return rc;
      for (const PlanKw& k : T.kws)
        if (k.tp_kind < 0 || k.tp_kind > MRK_TERMPOS_LIMIT || (k.tp_kind == MRK_TERMPOS_LIMIT && k.tp_max <= 0))
          return mrk_fail(MRK_E_INVAL, "query %u: bad position modifier", qi);
    }
    if (T.phrase || T.ph_leaf) {
      if (int rc = needs_hit_refs("PHRASE runs")) return rc;
      if (int rc = needs_rowids_31("hit")) return rc;
    }
    const bool weight_sum = (q.ranker == MRK_RANK_PROXIMITY_BM25 || q.ranker == MRK_RANK_PROXIMITY) && single_word;
    switch (q.ranker) {
      case MRK_RANK_NONE:
      case MRK_RANK_BM25: ranker = (uint32_t)q.ranker; break;
      case MRK_RANK_PROXIMITY_BM25:
      case MRK_RANK_PROXIMITY:
      case MRK_RANK_WORDCOUNT:
      case MRK_RANK_MATCHANY:
      case MRK_RANK_FIELDMASK:
      case MRK_RANK_SPH04: {
        // a single keyword under a proximity ranker is ranked by ExtRanker_WeightSum_c (sphinxsearch.cpp:4195-4196, 4216-4217)
        if (weight_sum) {
          ranker = q.ranker == MRK_RANK_PROXIMITY_BM25 ? MRK_RANK_BM25 : MRK_RANK_PROXIMITY;
          if (ranker == MRK_RANK_PROXIMITY && !use_packed)
            return mrk_fail(MRK_E_UNSUPPORTED, "query %u: ranker=proximity runs on the packed path only", qi);
          break;
        }
        // the others are always ExtRanker_State_T over the hit stream, single keyword or not (sphinxsearch.cpp:4214-4236)
        const bool proximity = q.ranker == MRK_RANK_PROXIMITY_BM25 || q.ranker == MRK_RANK_PROXIMITY;
        if (int rc = needs_hit_refs(proximity ? "proximity rankers run" : "hit rankers run")) return rc;
        if (n > MAX_PROX_TERMS && !gen)
          return mrk_fail(MRK_E_UNSUPPORTED, proximity ? "query %u: proximity over %d keywords (device path: <= %d)" : "query %u: hit ranker over %d keywords (device path: <= %d)", qi, n, MAX_PROX_TERMS);
        if (int rc = needs_rowids_31(proximity ? "proximity" : "hit")) return rc;
        if (T.multiand3_inner && !gen) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: 3-keyword AND below another operator with a hit ranker", qi);
        ranker = (uint32_t)q.ranker;
        prox = true;
        break;
      }
      default: return mrk_fail(MRK_E_UNSUPPORTED, "query %u: ranker %d not on the device path", qi, q.ranker);
    }
    return MRK_OK;
  }

  // The specialised paths first; a shape they decline goes to the generic per-doc evaluator (mrk_keval.h) when the segment
  // has what it reads (packed doclists + hit references), else the decline stands.
  int shape_query() {
    int rc = shape(false);
    if (rc == MRK_E_UNSUPPORTED && use_packed && seg->dev.pk_hit) {
      char fast_msg[256];
      snprintf(fast_msg, sizeof fast_msg, "%s", mrk_last_error());
      rc = shape(true);
      if (rc == MRK_E_UNSUPPORTED) { // both declined: say why, the specialised path's reason first
        char gen_msg[256];
        snprintf(gen_msg, sizeof gen_msg, "%s", mrk_last_error());
        return mrk_fail(MRK_E_UNSUPPORTED, "%s; generic evaluator: %s", fast_msg, gen_msg);
      }
    }
    return rc;
  }

  // One mrk_filter as the kernels read it: a row attribute, a multi-value attribute in the blob pool, or (on_weight) the match weight,
  // whose locator fields are ignored
  int translate_filter(const mrk_filter& f, bool on_weight, DevFilter& d) const {
    memset(&d, 0, sizeof d);
    if (on_weight) {
      if (f.kind != MRK_FILTER_VALUES && f.kind != MRK_FILTER_RANGE) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: weight filter kind %d", qi, f.kind);
    } else {
      if (f.kind != MRK_FILTER_VALUES && f.kind != MRK_FILTER_RANGE && f.kind != MRK_FILTER_FLOATRANGE)
        return mrk_fail(MRK_E_UNSUPPORTED, "query %u: filter kind %d not on the device path", qi, f.kind);
      if (f.kind == MRK_FILTER_FLOATRANGE && f.bit_count != 32) return mrk_fail(MRK_E_INVAL, "query %u: a float filter needs a 32-bit attribute", qi);
    }
    const bool in_row = !on_weight && !f.mva_bits;
    if (!on_weight && f.mva_bits) { // a multi-value attribute in the blob pool
      if (f.mva_bits != 32 && f.mva_bits != 64) return mrk_fail(MRK_E_INVAL, "query %u: MVA width %d", qi, f.mva_bits);
      if (f.kind == MRK_FILTER_FLOATRANGE) return mrk_fail(MRK_E_INVAL, "query %u: a float range over an MVA", qi);
      if (!seg->dev.blobs) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: MVA filters need the segment's blob pool (mrk_segment_set_blobs)", qi);
      if (f.n_blob_attrs < 1 || f.n_blob_attrs > 255 || f.blob_attr_id < 0 || f.blob_attr_id >= f.n_blob_attrs || (uint32_t)f.n_blob_attrs != seg->n_blob_attrs)
        return mrk_fail(MRK_E_INVAL, "query %u: blob attribute %d of %d (the segment's rows hold %u)", qi, f.blob_attr_id, f.n_blob_attrs, seg->n_blob_attrs);
      if (seg->dev.attr_stride < 4) return mrk_fail(MRK_E_INVAL, "query %u: rows of %u dwords hold no blob locator", qi, seg->dev.attr_stride);
      d.mva = (uint32_t)f.mva_bits | (f.mva_all ? 1u << 8 : 0) | ((uint32_t)f.blob_attr_id << 16) | ((uint32_t)f.n_blob_attrs << 24);
    } else if (in_row) {
      const bool wide = f.bit_count == 64;
      if (f.bit_offset < 0 || f.bit_count < 1 || (!wide && (f.bit_count > 32 || (f.bit_offset & 31) + f.bit_count > 32)) || (wide && (f.bit_offset & 31)) ||
          (uint64_t)f.bit_offset + (uint64_t)f.bit_count > (uint64_t)seg->dev.attr_stride * 32)
        return mrk_fail(MRK_E_INVAL, "query %u: filter locator %d/%d outside the %u-dword row", qi, f.bit_offset, f.bit_count, seg->dev.attr_stride);
      d.item = (uint32_t)f.bit_offset >> 5;
      d.shift = (uint32_t)f.bit_offset & 31u;
      d.bits = (uint32_t)f.bit_count;
    }
    d.kind = (uint32_t)f.kind | (f.exclude ? 1u << 8 : 0) | (f.has_equal_min ? 1u << 9 : 0) | (f.has_equal_max ? 1u << 10 : 0);
    if (in_row) d.kind |= (f.open_left ? 1u << 11 : 0) | (f.open_right ? 1u << 12 : 0);
    d.lo = f.min_value, d.hi = f.max_value;
    if (in_row && f.kind == MRK_FILTER_FLOATRANGE) { // the bounds travel as their bit patterns
      uint32_t lo_bits, hi_bits;
      memcpy(&lo_bits, &f.fmin, 4), memcpy(&hi_bits, &f.fmax, 4);
      d.lo = lo_bits, d.hi = hi_bits;
    }
    if (f.kind == MRK_FILTER_VALUES) {
      if (f.n_values < 1 || !f.values) return mrk_fail(MRK_E_INVAL, "query %u: values filter without values", qi);
      if (f.n_values > MRK_MAX_FILTER_VALUES) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: %d filter values (device path: <= %d)", qi, f.n_values, MRK_MAX_FILTER_VALUES);
      d.n_values = (uint32_t)f.n_values;
      for (int k = 0; k < f.n_values; ++k) d.values[k] = f.values[k];
    }
    return MRK_OK;
  }

  // A filter list of the query: attribute filters (EarlyReject: resolved locators over the segment's .spa rows), or filters on the
  // match weight (m_pWeightFilter: evaluated where a match's weight is final)
  int translate_filters(const char* noun, const mrk_filter* list, int32_t count, bool on_weight, DevFilter* out, uint32_t& n_out) const {
    n_out = 0;
    if (count < 0 || (count > 0 && !list)) return mrk_fail(MRK_E_INVAL, "query %u: bad %s list", qi, noun);
    if (count == 0) return MRK_OK;
    if (!on_weight && !seg->dev.attrs) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: filters need the segment's attribute rows (mrk_segment_set_attrs)", qi);
    if (!use_packed) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: %ss run on the packed path only", qi, noun);
    if (count > MRK_MAX_FILTERS) return mrk_fail(MRK_E_UNSUPPORTED, "query %u: %d %ss (device path: <= %d)", qi, count, noun, MRK_MAX_FILTERS);
    for (int i = 0; i < count; ++i)
      if (int rc = translate_filter(list[i], on_weight, out[i])) return rc;
    n_out = (uint32_t)count;
    return MRK_OK;
  }

  // ExtRanker_c::m_iMaxQpos = GetQwords() (sphinxsearch.cpp:4294-4296, 4372)
  // ... over the keywords the query does not EXCLUDE: TagExcluded (sphinx.cpp:15107-15129) marks the words on the right of an
  // ANDNOT, toggling with every nesting, and an excluded word's GetQwords() answers -1 (searchnode.cpp:2039, 2053).  (The tree
  // was walked by build_tree / build_gen before: it is a tree of at most PLAN_CAP nodes.)
  static uint32_t max_query_pos(const mrk_query& q, const PlanTree& T) {
    std::vector<uint8_t> ex((size_t)q.n_nodes, 0);
    struct Walk {
      const mrk_query& q;
      std::vector<uint8_t>& ex;
      void go(int32_t ni, bool neg, int depth) {
        if (ni < 0 || ni >= q.n_nodes || depth > 16) return;
        const mrk_node& nd = q.nodes[ni];
        if (nd.op == MRK_OP_TERM) {
          ex[(size_t)ni] = neg ? 1 : 0;
          return;
        }
        if (nd.n_children < 0 || nd.first_child < 0) return;
        for (int i = 0; i < nd.n_children; ++i) go(q.children[nd.first_child + i], (nd.op == MRK_OP_ANDNOT && i == 1) ? !neg : neg, depth + 1);
      }
    } walk{q, ex};
    walk.go(q.root, false, 0);
    uint32_t max_qpos = 0;
    for (const PlanKw& k : T.kws)
      if (!k.hidden && !(k.node >= 0 && k.node < q.n_nodes && ex[(size_t)k.node])) max_qpos = std::max<uint32_t>(max_qpos, (uint32_t)std::max(k.atom_pos, 0));
    return max_qpos;
  }

  // IDFs: distinct words in GetQwords traversal order (searchnode.cpp:2029-2055, 3276-3286); then what the ranker reads of the query
  void weigh_words(DevQuery& dq) {
    for (int i = 0; i < n; ++i) {
      if (T.kws[i].hidden) { // read for its hits only
        T.kws[i].weighted_first = false;
        continue;
      }
      bool seen = false;
      for (int w : words) seen |= T.kws[i].term_id >= 0 && T.kws[w].term_id == T.kws[i].term_id; // words missing from the dictionary are distinct words
      T.kws[i].weighted_first = !seen;
      if (!seen) words.push_back(i);
    }
    int n_visible = 0;
    for (const PlanKw& k : T.kws) n_visible += k.hidden ? 0 : 1;
    got_dupes = (int)words.size() != n_visible; // HasQwordDupes: proximity rankers switch to their HANDLE_DUPES update
    const int64_t total_docs = q.total_docs_override > 0 ? q.total_docs_override : (int64_t)seg->total_docs;
    for (int w : words) {
      PlanKw& t = T.kws[w];
      int64_t term_docs = t.docs;
      if (q.local_docs && q.local_docs[t.node] >= 0) term_docs = q.local_docs[t.node];
      t.idf = mrk_idf(term_docs, total_docs, q.plain_idf, q.normalized_tfidf, (int)words.size(), t.boost);
    }
    dq.ranker = ranker;
    dq.n_qwords = (uint32_t)words.size(); // ExtRanker_c::m_iQwords (sphinxsearch.cpp:730-731)
    dq.max_qpos = max_query_pos(q, T);
    dq.k = (uint32_t)q.max_matches;
    dq.n_weights = seg->n_fields;
    dq.index_weight = (uint32_t)(q.index_weight ? q.index_weight : 1);
    for (uint32_t f = 0; f < 32; ++f)
      dq.weights[f] = (q.field_weights && (int)f < q.n_weights) ? q.field_weights[f] : 1; // BindWeights default
  }

  // The passes' drivers (one per keyword of the tree's candidate cover), the keywords no match goes without, what the scan reads
  int choose_cover() {
    IntVec all;
    if (pure_and)
      all.push_back(0); // kws are already in ExtMultiAnd_T node order: the rarest keyword drives
    else
      cover_of(T, root, all);
    for (int k : all)
      if (std::find(cover.begin(), cover.end(), k) == cover.end()) cover.push_back(k);
    if ((int)cover.size() > MAX_PASSES)
      return mrk_fail(MRK_E_UNSUPPORTED, "query %u: %zu driver keywords (device path: <= %d)", qi, cover.size(), MAX_PASSES);
    req = pure_and ? (n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u) : required_of(T, root);
    for (int k = 0; k < n; ++k)
      if ((req >> k & 1u) && !T.kws[k].docs) empty = true; // a required keyword without postings (searchnode.cpp:2922)
    for (int k = 0; k < n; ++k)
      if (T.kws[k].docs) {
        bytes += seg->terms[T.kws[k].term_id].doclist_len;
        pbytes += seg->terms[T.kws[k].term_id].packed_bytes;
      }
    return MRK_OK;
  }

  // ---- pruning histogram geometry (packed path): bins must be monotone in the sorter's order

  // the least shift that brings `span` under NBINS bins
  static uint32_t bin_shift_for(uint64_t span) {
    uint32_t sh = 0;
    while (sh < 31 && (span >> sh) >= (uint64_t)NBINS) ++sh;
    return sh;
  }

  // all weights equal: order is rowid ascending => bin on the (global) rowid
  static void bins_by_rowid(const mrk_segment* seg, DevQuery& dq) {
    dq.bin_mode = BIN_ROWID;
    const uint64_t max_row = (uint64_t)seg->dev.rowid_base + (seg->total_docs ? seg->total_docs : 1);
    dq.bin_shift = max_row > 0xFFFFFFFFull ? 22 : bin_shift_for(max_row);
    dq.bin_lo = 0;
  }

  // weight = ((int)((sum tfidf + 0.5f) * 1000) + rank * 1000) * index_weight; any keyword may be absent
  void bins_by_weight(DevQuery& dq) const {
    dq.bin_mode = BIN_WEIGHT;
    dq.bin_lo = INT32_MIN;
    dq.bin_shift = 31; // fallback: (almost) no pruning, always correct
    double lo = 0.0, hi = 0.0;
    for (int i = 0; i < n; ++i) {
      const double idf = T.kws[i].weighted_first ? T.kws[i].idf : 0.0;
      const double a0 = idf * (1.0 / 2.2), a1 = idf;
      lo += std::min(0.0, std::min(a0, a1));
      hi += std::max(0.0, std::max(a0, a1));
      if (pure_and) { // every keyword contributes
        lo += std::min(a0, a1) - std::min(0.0, std::min(a0, a1));
        hi += std::max(a0, a1) - std::max(0.0, std::max(a0, a1));
      }
    }
    // (a boost of inf / NaN makes the weights meaningless in the reference too; the estimate just must stay defined)
    lo = std::isfinite(lo) ? std::max(lo, -1e12) : -1e12;
    hi = std::isfinite(hi) ? std::min(hi, 1e12) : 1e12;
    const int64_t bm_lo = (int64_t)floor((lo + 0.5) * 1000.0) - 2, bm_hi = (int64_t)ceil((hi + 0.5) * 1000.0) + 2;
    int64_t rmin = INT64_MAX, rmax = INT64_MIN;
    const uint32_t nwf = std::min<uint32_t>(dq.n_weights, seg->wide ? 32u : 8u);
    if (prox) {
      // sum_f LCS[f] * w[f] with 0 <= LCS[f] <= number of keywords (hit weight 1, unique keywords)
      // (a phrase occurrence weighs its word count; back-to-back occurrences can add up -- beyond 2n the bins clamp)
      // The other state rankers: SPH04 4*LCS + 2 + 1 per field; WORDCOUNT one field weight per hit (unbounded:
      // 32 hits per keyword span the bins, more clamp); MATCHANY bits + (LCS-1) * K, K = sum(w) * words;
      // FIELDMASK the mask itself.  Bounds only shape the pruning bins -- values outside clamp to the edge bins.
      rmin = rmax = 0;
      int64_t top = (T.phrase || T.ph_leaf || T.gen) ? 2 * n : n;
      if (ranker == MRK_RANK_SPH04) top = 4 * top + 3;
      if (ranker == MRK_RANK_WORDCOUNT) top = 32 * n;
      if (ranker == MRK_RANK_MATCHANY) {
        int64_t k = 0;
        for (uint32_t f = 0; f < nwf; ++f) k += dq.weights[f];
        top = sat_add(n, sat_mul(top, std::llabs(sat_mul(k, (int64_t)words.size()))));
      }
      for (uint32_t f = 0; f < nwf; ++f) {
        const int64_t v = sat_mul(top, dq.weights[f]);
        rmin = sat_add(rmin, ranker == MRK_RANK_MATCHANY ? -std::llabs(v) : std::min<int64_t>(0, v));
        rmax = sat_add(rmax, ranker == MRK_RANK_MATCHANY ? std::llabs(v) : std::max<int64_t>(0, v));
      }
      if (ranker == MRK_RANK_FIELDMASK) rmin = 0, rmax = (1ll << nwf) - 1;
    } else
      weight_sum_range(dq.weights, nwf, rmin, rmax);
    const bool with_bm = ranker == MRK_RANK_BM25 || ranker == MRK_RANK_PROXIMITY_BM25 || ranker == MRK_RANK_SPH04;
    const int64_t iw = (int32_t)dq.index_weight;
    const int64_t sc = with_bm ? 1000 : 1, b0 = with_bm ? bm_lo : 0, b1 = with_bm ? bm_hi : 0;
    // (128-bit: absurd field weights x an absurd index weight must not overflow the estimate itself)
    const __int128 c[4] = {((__int128)b0 + (__int128)rmin * sc) * iw, ((__int128)b0 + (__int128)rmax * sc) * iw, ((__int128)b1 + (__int128)rmin * sc) * iw,
                           ((__int128)b1 + (__int128)rmax * sc) * iw};
    const __int128 wlo = *std::min_element(c, c + 4), whi = *std::max_element(c, c + 4);
    if (wlo > INT32_MIN && whi < INT32_MAX && std::llabs(rmin) < INT32_MAX / 1000 && std::llabs(rmax) < INT32_MAX / 1000) {
      dq.bin_lo = (int32_t)wlo;
      dq.bin_shift = bin_shift_for((uint64_t)(whi - wlo));
    }
  }

  // a column's range of mapped keys in the query's direction: no rows = 0..0; ascending: the keys are complemented
  template <typename U>
  static void directed(U& lo, U& hi, bool desc) {
    if (lo > hi) lo = hi = 0;
    if (!desc) {
      const U l = ~hi, h = ~lo;
      lo = l, hi = h;
    }
  }

  // the order starts with an attribute: where the key lies in the row, and the bins over the column's range of mapped keys
  static void bins_by_key(const KeySpec& O, DevQuery& dq) {
    const KeyPart &A = O.part[0], &B = O.part[O.n_parts - 1];
    dq.sort_tie = (uint32_t)O.tie;
    dq.bin_mode = BIN_WEIGHT;
    dq.sort_item = A.item(), dq.sort_shift = (uint32_t)A.bit_offset & 31u, dq.sort_bits = (uint32_t)A.bit_count, dq.sort_flags = A.flags();
    if (!O.wide) { // (bin_lo read as unsigned)
      dq.sort_on = SORT_ON_ATTR;
      uint32_t lo = A.range->lo, hi = A.range->hi;
      directed(lo, hi, A.desc);
      dq.bin_lo = (int32_t)lo;
      dq.bin_shift = bin_shift_for(hi - lo);
      return;
    }
    // a 64-bit key: two dwords of the row, the compressed bins of mrk_sortkey.h
    const bool i64 = A.kind == MRK_SORTKEY_INT64;
    dq.sort_on = SORT_ON_ORDER;
    uint32_t a_lo, a_hi, b_lo, b_hi;
    if (i64) { // high dword signed, low dword unsigned, one direction
      dq.sort_item = A.item() + 1, dq.sort_shift = 0, dq.sort_bits = 32, dq.sort_flags = A.flags() | SORT_SIGNED;
      dq.ord_item = A.item(), dq.ord_shift = 0, dq.ord_bits = 32, dq.ord_flags = A.flags();
      uint64_t lo = A.range->lo64, hi = A.range->hi64;
      directed(lo, hi, A.desc);
      a_lo = (uint32_t)(lo >> 32), b_lo = (uint32_t)lo, a_hi = (uint32_t)(hi >> 32), b_hi = (uint32_t)hi;
    } else {
      dq.ord_item = B.item(), dq.ord_shift = (uint32_t)B.bit_offset & 31u, dq.ord_bits = (uint32_t)B.bit_count, dq.ord_flags = B.flags();
      a_lo = A.range->lo, a_hi = A.range->hi, b_lo = B.range->lo, b_hi = B.range->hi;
      directed(a_lo, a_hi, A.desc), directed(b_lo, b_hi, B.desc);
    }
    dq.ord_geom = order_geom(a_lo, a_hi, b_lo, b_hi, i64);
    dq.sort_flags |= SORT_WIDE;
    dq.bin_lo = 0, dq.bin_shift = 0;
  }

  // the weight leads the order (MRK_ORDER_WEIGHT_FIRST_*): the relevance bins of the weight -- the kernels complement the bin for weight
  // ASC --, and behind it where the parts lie in the row: 0..2 dwords (a 64-bit attribute: high, low), no geometry of theirs.  A ranker
  // whose weights are all equal (NONE) fills one bin: correct, through the list overflow and the rerun, and not fast
  void bins_by_weight_first(DevQuery& dq) const {
    const KeySpec& O = order;
    bins_by_weight(dq);
    dq.sort_on = SORT_ON_WEIGHT;
    dq.sort_tie = (uint32_t)O.wfirst;
    dq.sort_flags = SORT_WFIRST;
    if (O.n_parts) {
      const KeyPart &A = O.part[0], &B = O.part[O.n_parts - 1];
      if (A.kind == MRK_SORTKEY_INT64) {
        dq.sort_item = A.item() + 1, dq.sort_shift = 0, dq.sort_bits = 32, dq.sort_flags |= A.flags() | SORT_SIGNED;
        dq.ord_item = A.item(), dq.ord_shift = 0, dq.ord_bits = 32, dq.ord_flags = A.flags();
        dq.wf_parts = 2;
      } else {
        dq.sort_item = A.item(), dq.sort_shift = (uint32_t)A.bit_offset & 31u, dq.sort_bits = (uint32_t)A.bit_count, dq.sort_flags |= A.flags();
        if (O.n_parts == 2) dq.ord_item = B.item(), dq.ord_shift = (uint32_t)B.bit_offset & 31u, dq.ord_bits = (uint32_t)B.bit_count, dq.ord_flags = B.flags();
        dq.wf_parts = (uint32_t)O.n_parts;
      }
    }
  }

  // the query's candidate list: a slot range of the batch's arena (16-byte candidates in the arena of the sorted queries; the
  // relevance selection sees an empty list)
  void reserve_candidates(DevQuery& dq, BatchPlan& plan) const {
    uint64_t cap = 0;
    for (int k : cover) cap += (uint64_t)T.kws[k].docs;
    cap = std::min<uint64_t>(std::max<uint64_t>(cap, 1), (uint64_t)1 << 20);
    dq.cand_off = plan.cand_total;
    if (order.sorted()) {
      dq.cand_cap = 0;
      dq.sort_cap = (uint32_t)cap;
      dq.sort_off = plan.sort_total;
      plan.sort_total += cap;
    } else {
      dq.cand_cap = (uint32_t)cap;
      plan.cand_total += cap;
    }
  }

  // ---- the bitmap-driven kernels: whole window ranges instead of block ranges

  // the tree program: op | left node << 8 | right node << 16 | keyword << 24 (slot: the pass's keyword order; none = the tree's)
  static void pack_prog(const PlanTree& T, const IntVec* slot, DevQuery& P) {
    P.n_nodes = (uint32_t)T.nodes.size();
    for (size_t i = 0; i < T.nodes.size(); ++i) {
      const PlanNode& pn = T.nodes[i];
      const int kw = pn.kw < 0 ? 0 : slot ? (*slot)[pn.kw] : pn.kw;
      P.prog[i] = pn.op | ((uint32_t)(pn.l < 0 ? 0 : pn.l) << 8) | ((uint32_t)(pn.r < 0 ? 0 : pn.r) << 16) | ((uint32_t)kw << 24);
    }
  }

  // One entry for the pass's whole window range; layout_batch cuts it once the batch's total is known (a wave's fixed costs --
  // tables, final publish, atomics on the query's counters -- want long runs of windows).  dev_bytes: what the kernel reads instead
  // of the packed blocks counted before
  void emit_window_item(DevQuery& P, uint32_t pass_index, uint32_t kind, uint64_t dev_bytes, BatchPlan& plan) const {
    P.item_first = (uint32_t)plan.items_bm.size();
    plan.dev_bytes += dev_bytes - pbytes;
    DevItem it{};
    it.query = pass_index;
    it.blk_begin = 0;
    it.blk_end = (uint32_t)seg->dev.n_windows;
    it.kind = kind;
    plan.items_bm.push_back(it);
    P.n_items = 1;
  }

  // what the three kernels share: the packed path of a segment with doc-set bitmaps, nothing that reads attribute rows or weights
  bool bitmaps_usable() const {
    return use_packed && seg->dev.bm && !seg->wide && seg->ctx->bitmap_inv > 0 && !filtered && q.n_weight_filters == 0;
  }
  bool is_dense(int k) const { return T.kws[k].docs && seg->terms[T.kws[k].term_id].bm_off != ~0ull; }

  // ... and the tree kernel's two uses (mrk_scan_bt.hip): a plain tree whose cover is common enough (cover_inv: 1 / the least share of
  // the docs), every keyword unrestricted in fields (a bitmap bit is then "the keyword holds the doc"), one of them dense (sparse
  // keywords are fine, their window words are assembled from a block cursor)
  bool tree_kernel_usable(int cover_inv) const {
    if (!bitmaps_usable() || seg->ctx->bt_cover_inv <= 0 || T.gen || T.ph_leaf || T.quorum || T.order || T.termpos || T.notnear || n > MAX_PROX_TERMS ||
        seg->total_docs >= (1ull << 32) || T.nodes.size() > 16)
      return false;
    uint64_t cover_docs = 0;
    for (int k : cover) cover_docs += (uint64_t)T.kws[k].docs;
    if (cover_docs * (uint64_t)cover_inv < seg->total_docs) return false;
    const uint32_t all_fields = seg->n_fields >= 32 ? 0xFFFFFFFFu : (1u << seg->n_fields) - 1u;
    int n_dense = 0;
    for (int k = 0; k < n; ++k) {
      if ((T.kws[k].queried32 & all_fields) != all_fields) return false;
      n_dense += is_dense(k);
    }
    return n_dense > 0 && stack_depth(T) <= TREE_STACK;
  }
  // bitmaps of the dense keywords + packed blocks of the sparse ones + every keyword's tf / field words
  uint64_t tree_kernel_bytes() const {
    uint64_t b = 0;
    for (int k = 0; k < n; ++k)
      if (T.kws[k].docs) {
        const HostTerm& h = seg->terms[T.kws[k].term_id];
        b += h.bm_off != ~0ull ? (uint64_t)seg->dev.n_windows * 256 + (uint64_t)h.nblocks * 256 : h.packed_bytes;
      }
    return b;
  }

  // two dense keywords: the bitmap kernel (mrk_scan_bm.hip) walks 2048-rowid windows instead of blocks
  bool pair_on_bitmaps(DevQuery& dq, BatchPlan& plan) const {
    if (!bitmaps_usable() || !pure_and || T.phrase || n != 2 || (ranker != MRK_RANK_NONE && ranker != MRK_RANK_BM25) || !is_dense(0) || !is_dense(1)) return false;
    dq.n_terms = 2;
    for (int i = 0; i < 2; ++i) fill_term(seg, T.kws[i], dq.t[i]);
    dq.tree_flags = TF_MULTIAND | TF_BITMAP;
    // bitmaps + tf / field bytes of the docs (one byte each where the segment has the nibble plane, else the attr words)
    const uint64_t bm_bytes = 2 * (uint64_t)seg->dev.n_windows * 256 + ((uint64_t)dq.t[0].nblocks + dq.t[1].nblocks) * (seg->dev.pk_attr1 ? 128 : 256);
    emit_window_item(dq, qi, 0, bm_bytes, plan);
    return true;
  }

  // A tree whose candidate cover is a common keyword: evaluate it on bitmap words, 2048 rowids per step, instead of
  // walking the cover's docs block by block (mrk_scan_bt.hip).
  // (a pure AND keeps the old bar of 1/32: below it the block walk behind a selective driver -- skiplist seeks, a probe per doc --
  // beats streaming every keyword's bitmap; with 1/1024 the headline's selective x common stratum went from 0.36 to 0.54 ms)
  bool tree_on_bitmaps(DevQuery& dq, BatchPlan& plan) const {
    const int bt_cover_inv = seg->ctx->bt_cover_inv;
    if (T.phrase || !tree_kernel_usable(pure_and ? std::min(bt_cover_inv, 32) : bt_cover_inv)) return false;
    dq.n_terms = (uint32_t)n;
    for (int i = 0; i < n; ++i) fill_term(seg, T.kws[i], dq.t[i]);
    dq.tree_flags = (pure_and ? TF_MULTIAND : 0) | (got_dupes ? TF_DUPES : 0) | TF_BTREE | (seg->ctx->prox_bound_keywords ? TF_LCS_BY_KEYWORDS : 0);
    pack_prog(T, nullptr, dq);
    emit_window_item(dq, qi, 1, tree_kernel_bytes(), plan);
    return true;
  }

  // A root PHRASE / PROXIMITY whose words are common: the AND of its words -- the candidates the word state machine has to look
  // at -- comes off the doc-set bitmaps, 8192 rowids per step (scan_bt_kernel), instead of the rarest word's blocks one by one
  // with a probe per doc and word; the candidates travel through the same queue to the same hit pass (rank_kernel<1>).
  // Config 5's phrase fifth spent 20 of its 36 ms per launch in the block walk.
  bool phrase_on_bitmaps(DevQuery& P, uint32_t pass_index, BatchPlan& plan) const {
    if (!T.phrase || cover.size() != 1 || !seg->ctx->bt_phrase || !pure_and || got_dupes || n < 2 || !tree_kernel_usable(seg->ctx->bt_cover_inv)) return false;
    P.tree_flags |= TF_BTREE | TF_MULTIAND;
    emit_window_item(P, pass_index, 1, tree_kernel_bytes(), plan);
    return true;
  }

  // ---- the block scan's passes

  // ExtQuorum_c's m_dChildren over time: query-position order; a keyword leaves (RemoveFast: the last one takes its place) once the
  // doc it sits on was its last -- keywords without docs right at the warmup (searchnode.cpp:4468-4483, 4517-4537)
  void quorum_schedule(const IntVec& slot, DevQuery& P) const {
    P.qr_thr = (uint32_t)T.q_thr;
    if (T.quorum_root && prox) P.tree_flags |= TF_QUORUM_HITS;
    int list[QUORUM_EVENTS], ln = T.q_n;
    for (int i = 0; i < ln; ++i) list[i] = T.q_kw0 + i, P.qr_mask |= 1u << slot[T.q_kw0 + i];
    auto pack_order = [&]() {
      uint32_t o = 0xFFFFFFFFu;
      for (int i = ln - 1; i >= 0; --i) o = (o << 4) | (uint32_t)slot[list[i]];
      return o;
    };
    auto last_of = [&](int k) -> int64_t { return T.kws[k].docs ? (int64_t)seg->terms[T.kws[k].term_id].last_rowid : -1; };
    for (int i = 0; i < ln; ++i) // warmup: keywords that hold no doc at all
      if (last_of(list[i]) < 0) {
        list[i] = list[--ln];
        --i;
      }
    P.qr_ord[0] = pack_order();
    while (ln > 0 && P.qr_n < (uint32_t)QUORUM_EVENTS) {
      int64_t r = INT64_MAX;
      for (int i = 0; i < ln; ++i) r = std::min(r, last_of(list[i]));
      for (int i = 0; i < ln; ++i)
        if (last_of(list[i]) == r) {
          list[i] = list[--ln];
          --i;
        }
      P.qr_row[P.qr_n] = (uint32_t)r;
      P.qr_ord[++P.qr_n] = pack_order();
    }
  }

  // the evaluator's program, keyword slots as the pass orders them
  static void remap_gen_prog(GenProg& gp, const IntVec& slot) {
    for (uint32_t i = 0; i < gp.n_nodes; ++i) {
      GenNode& g = gp.nodes[i];
      if (g.kind == GN_TERM) g.kid[0] = (uint8_t)slot[g.kid[0]];
      if (g.kind == GN_MULTIAND || g.kind == GN_QUORUM)
        for (int k = 0; k < g.n_kids; ++k) g.kid[k] = (uint8_t)slot[g.kid[k]];
      if (g.kind == GN_PHRASE || g.kind == GN_PROX)
        for (int k = 0; k < g.n_words; ++k) g.aux[k] = (uint8_t)slot[g.aux[k]];
      if (g.kind == GN_UNIT && g.aux[0] != 0xFF) g.aux[0] = (uint8_t)slot[g.aux[0]];
    }
  }

  // One pass per driver keyword of the cover: dq is the first, the others are copies of it in plan.extra
  void emit_passes(DevQuery& dq, int64_t item_bytes, uint32_t n_queries, BatchPlan& plan) const {
    DevQuery base_copy; // (1.3 KB: only copied when the query runs as several passes)
    if (cover.size() > 1) base_copy = dq;
    const DevQuery& base = base_copy;
    for (size_t p = 0; p < cover.size(); ++p) {
      DevQuery* P = &dq;
      uint32_t pass_index = qi;
      if (p > 0) {
        plan.extra.push_back(base);
        P = &plan.extra.back();
        pass_index = n_queries + (uint32_t)plan.extra.size() - 1;
        P->item_first = (uint32_t)plan.items.size();
      }
      if (T.gen) P->item_first = (uint32_t)plan.items_bm.size(), P->n_items = 0;
      // keyword order of this pass: driver, then required keywords by ascending docs, then the rest
      IntVec order;
      const int drv = cover[p];
      order.push_back(drv);
      if (pure_and)
        for (int k = 1; k < n; ++k) order.push_back(k);
      else {
        IntVec rq, rest;
        for (int k = 0; k < n; ++k)
          if (k != drv) ((req >> k & 1u) ? rq : rest).push_back(k);
        auto by_docs = [&](int a, int b) { return T.kws[a].docs < T.kws[b].docs; };
        std::stable_sort(rq.begin(), rq.end(), by_docs);
        std::stable_sort(rest.begin(), rest.end(), by_docs);
        order.append(rq.begin(), rq.end());
        order.append(rest.begin(), rest.end());
      }
      IntVec slot(n);
      for (int i = 0; i < n; ++i) slot[order[i]] = i;
      P->n_terms = (uint32_t)n;
      for (int i = 0; i < n; ++i) fill_term(seg, T.kws[order[i]], P->t[i]);
      P->req_mask = P->excl_mask = 0;
      P->tree_flags = (T.phrase ? TF_PHRASE : pure_and ? TF_MULTIAND : T.ph_leaf ? TF_PHRASE_LEAF : 0) | (got_dupes ? TF_DUPES : 0) | (T.termpos ? TF_TERMPOS : 0) | (T.order ? TF_ORDER : 0) | (T.notnear ? TF_NOTNEAR : 0) | (T.gen ? TF_GEN : 0) | (T.gen_nearn ? TF_GEN_NEARN : 0);
      if (T.gen) {
        P->gen_prog = (uint32_t)plan.gen_progs.size();
        plan.gen_progs.push_back(gen_build->prog);
        remap_gen_prog(plan.gen_progs.back(), slot);
      }
      P->nn_a = T.notnear ? (uint32_t)slot[T.nn_a] : 0u, P->nn_b = T.notnear ? (uint32_t)slot[T.nn_b] : 0u, P->nn_dist = (uint32_t)T.nn_dist;
      P->px_dist = (uint32_t)T.px_dist;
      P->qr_mask = P->qr_thr = P->qr_n = 0;
      if (T.quorum) quorum_schedule(slot, *P);
      P->ph_mask = 0;
      for (int k = 0; k < T.ph_n; ++k) P->ph_mask |= 1u << slot[T.ph_kw0 + k];
      for (size_t i = 0; i < T.atoms.size(); ++i) P->ph_atoms[i] = (uint32_t)T.atoms[i];
      for (int k = 0; k < n; ++k)
        if (req >> k & 1u) P->req_mask |= 1u << slot[k];
      for (size_t e = 0; e < p; ++e) P->excl_mask |= 1u << slot[cover[e]];
      pack_prog(T, &slot, *P);
      if (phrase_on_bitmaps(*P, pass_index, plan)) continue;
      // work items: contiguous ranges of driver-term blocks, ~item_bytes of doclist each
      const uint32_t nb0 = P->t[0].nblocks;
      if (nb0) {
        const double per_block = (double)(use_packed ? pbytes : bytes) / (double)nb0 / (double)cover.size();
        uint64_t bpi = (uint64_t)((double)item_bytes / std::max(per_block, 1.0));
        bpi = std::max<uint64_t>(T0_BLOCKS, (bpi / T0_BLOCKS) * T0_BLOCKS);
        for (uint64_t b = 0; b < nb0; b += bpi) {
          DevItem it{};
          it.query = pass_index;
          it.blk_begin = (uint32_t)b;
          it.blk_end = (uint32_t)std::min<uint64_t>(nb0, b + bpi);
          if (T.gen) { // its own launch (the scan instance that hands over a reference per keyword), behind the block items
            it.kind = 2;
            plan.items_bm.push_back(it);
            ++P->n_items;
          } else
            plan.items.push_back(it);
        }
      }
      if (!T.gen) P->n_items = (uint32_t)plan.items.size() - P->item_first;
    }
  }
};

int mrk::plan_query(const mrk_segment* seg, const mrk_query& q, int64_t item_bytes, bool use_packed, DevQuery& dq, uint32_t n_queries, uint32_t qi,
                    BatchPlan& plan, uint32_t rowid_max, const mrk_group* group, const mrk_aggrs* aggrs, const mrk_group_mva* mva) {
  memset(&dq, 0, sizeof dq);
  PlanState S{seg, q, use_packed, qi, group, aggrs, mva};
  if (mva && !group) return mrk_fail(MRK_E_INVAL, "query %u: a multi-value group attribute without a group", qi);
  // validate: hostile order / sort specs are MRK_E_INVAL before a row is read
  if (int rc = S.resolve_order()) return rc;
  dq.item_first = (uint32_t)plan.items.size();
  dq.out_q = qi;
  if (int rc = S.check_query()) return rc;
  if (int rc = S.resolve_sort()) return rc;
  if (int rc = S.check_aggrs()) return rc;
  if (int rc = S.resolve_group()) return rc;
  if (int rc = S.decline_aggrs()) return rc;
  // (a sorted or grouped query reads attribute rows like a filtered one: the packed block scan's EXT instances only)
  S.filtered = q.n_filters > 0 || rowid_max != 0xFFFFFFFFu || S.order.sorted() || group != nullptr;
  // the evaluation tree and who evaluates it
  if (int rc = S.shape_query()) return rc;
  dq.rowid_max = rowid_max;
  if (int rc = S.translate_filters("filter", q.filters, q.n_filters, false, dq.filters, dq.n_filters)) return rc;
  if (int rc = S.translate_filters("weight filter", q.weight_filters, q.n_weight_filters, true, dq.wfilters, dq.n_wfilters)) return rc;
  S.weigh_words(dq);
  if (int rc = S.choose_cover()) return rc;
  // pruning bins and the candidate list
  if (S.order.wfirst)
    S.bins_by_weight_first(dq);
  else if (S.order.n_parts)
    PlanState::bins_by_key(S.order, dq);
  else if (S.ranker == MRK_RANK_NONE)
    PlanState::bins_by_rowid(seg, dq);
  else
    S.bins_by_weight(dq);
  if (group)
    S.reserve_group(dq, plan);
  else
    S.reserve_candidates(dq, plan);
  if (S.empty) {
    dq.n_terms = (uint32_t)S.n;
    dq.n_items = 0;
    return MRK_OK;
  }
  const PlanTree& T = S.T;
  plan.algo_bytes += S.bytes;
  plan.dev_bytes += use_packed ? S.pbytes : S.bytes;
  plan.any_prox = plan.any_prox || S.prox || T.phrase || T.ph_leaf || T.termpos || T.notnear || T.gen; // (every generic-path candidate goes through the queue)
  plan.any_tree = plan.any_tree || !S.pure_and;
  // passes and work items: a bitmap-driven kernel where one applies, else the block scan, one pass per driver keyword
  if (S.pair_on_bitmaps(dq, plan) || S.tree_on_bitmaps(dq, plan)) return MRK_OK;
  S.emit_passes(dq, item_bytes, n_queries, plan);
  return MRK_OK;
}

// ----------------------------------------------------------------------------------------

void mrk::plan_bm_groups(const std::vector<BmMember>& m, std::vector<uint32_t>& order, std::vector<uint32_t>& sizes) {
  order.clear(), sizes.clear();
  const uint32_t n = (uint32_t)m.size();
  // classes in the order of their first member; each class's members ascending
  std::vector<uint32_t> by_cls(n);
  for (uint32_t i = 0; i < n; ++i) by_cls[i] = i;
  std::vector<uint32_t> cls_rank(n, ~0u); // class rank by first appearance (cls values are arbitrary)
  {
    std::vector<std::pair<uint32_t, uint32_t>> seen; // (cls, rank)
    std::vector<uint32_t> rank(n);
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t r = ~0u;
      for (const auto& c : seen)
        if (c.first == m[i].cls) r = c.second;
      if (r == ~0u) r = (uint32_t)seen.size(), seen.emplace_back(m[i].cls, r);
      rank[i] = r;
    }
    std::stable_sort(by_cls.begin(), by_cls.end(), [&](uint32_t a, uint32_t b) { return rank[a] < rank[b]; });
    for (uint32_t i = 0; i < n; ++i) cls_rank[i] = rank[i];
  }
  std::vector<uint64_t> keys;
  std::vector<uint32_t> ka, kb, cnt, have, hold_first, hold;
  std::vector<uint64_t> kbytes;
  std::vector<uint8_t> done;
  for (uint32_t c0 = 0; c0 < n;) {
    uint32_t c1 = c0;
    while (c1 < n && cls_rank[by_cls[c1]] == cls_rank[by_cls[c0]]) ++c1;
    const uint32_t* mem = by_cls.data() + c0; // the class's members, ascending
    const uint32_t nm = c1 - c0;
    // dense key ids of the class, in key order (ties of the greedy go to the smaller key); a key's bytes are the class's
    keys.clear();
    for (uint32_t j = 0; j < nm; ++j) keys.push_back(m[mem[j]].key[0]), keys.push_back(m[mem[j]].key[1]);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const size_t nk = keys.size();
    ka.assign(nm, 0), kb.assign(nm, 0), done.assign(nm, 0);
    cnt.assign(nk, 0), have.assign(nk, 0), kbytes.assign(nk, 0), hold_first.assign(nk + 1, 0);
    for (uint32_t j = 0; j < nm; ++j) {
      const BmMember& x = m[mem[j]];
      ka[j] = (uint32_t)(std::lower_bound(keys.begin(), keys.end(), x.key[0]) - keys.begin());
      kb[j] = (uint32_t)(std::lower_bound(keys.begin(), keys.end(), x.key[1]) - keys.begin());
      kbytes[ka[j]] = x.bytes[0], kbytes[kb[j]] = x.bytes[1];
      ++cnt[ka[j]];
      if (kb[j] != ka[j]) ++cnt[kb[j]];
    }
    // holder lists (members ascending): hold[hold_first[k] .. hold_first[k + 1])
    for (size_t k = 0; k < nk; ++k) hold_first[k + 1] = hold_first[k] + cnt[k];
    hold.assign(hold_first[nk], 0);
    {
      std::vector<uint32_t> fill(hold_first.begin(), hold_first.end() - 1);
      for (uint32_t j = 0; j < nm; ++j) {
        hold[fill[ka[j]]++] = j;
        if (kb[j] != ka[j]) hold[fill[kb[j]]++] = j;
      }
    }
    uint32_t stamp = 0;
    for (;;) {
      // cnt[k] = holders of k not yet placed: the seed is the key most of them hold (ties: the smaller key)
      uint32_t best = 0;
      for (uint32_t k = 1; k < nk; ++k)
        if (cnt[k] > cnt[best]) best = k;
      if (nk == 0 || cnt[best] < 2) break;
      ++stamp;
      have[best] = stamp;
      const size_t g0 = order.size();
      while (order.size() - g0 < (size_t)BM_GROUP_MAX) {
        // the seed's holder that adds the fewest bytes of keys new to the group (ties: the lower index)
        uint32_t pick = ~0u;
        uint64_t pick_cost = 0;
        for (uint32_t h = hold_first[best]; h < hold_first[best + 1]; ++h) {
          const uint32_t j = hold[h];
          if (done[j]) continue;
          const uint64_t cost = (have[ka[j]] == stamp ? 0 : kbytes[ka[j]]) + (have[kb[j]] == stamp || kb[j] == ka[j] ? 0 : kbytes[kb[j]]);
          if (pick == ~0u || cost < pick_cost) pick = j, pick_cost = cost;
        }
        if (pick == ~0u) break;
        done[pick] = 1;
        have[ka[pick]] = have[kb[pick]] = stamp;
        --cnt[ka[pick]];
        if (kb[pick] != ka[pick]) --cnt[kb[pick]];
        order.push_back(mem[pick]);
      }
      sizes.push_back((uint32_t)(order.size() - g0));
    }
    for (uint32_t j = 0; j < nm; ++j) // no key of theirs is held by another member left: alone
      if (!done[j]) order.push_back(mem[j]), sizes.push_back(1);
    c0 = c1;
  }
}

bool mrk::pass_queues_matches(const DevQuery& P, bool& fat) {
  const uint32_t rk = P.ranker;
  if (P.tree_flags & mrk::TF_GEN) return fat = false, true; // (queue 2: see queue_of)
  const bool prox_ranker = (rk == MRK_RANK_PROXIMITY_BM25 || rk == MRK_RANK_PROXIMITY)
                               ? P.n_terms > 1
                               : (rk == MRK_RANK_WORDCOUNT || rk == MRK_RANK_MATCHANY || rk == MRK_RANK_FIELDMASK || rk == MRK_RANK_SPH04);
  fat = (P.tree_flags & mrk::TF_FAT) != 0;
  return prox_ranker || (P.tree_flags & mrk::TF_PHRASE) != 0;
}

int mrk::queue_of(const DevQuery& P, bool fat) { return (P.tree_flags & mrk::TF_GEN) ? 2 : fat ? 1 : 0; }

uint64_t mrk::pass_max_matches(const DevQuery& P) {
  if (P.tree_flags & mrk::TF_BITMAP) return std::min<uint64_t>(P.t[0].docs, P.t[1].docs);
  if (P.tree_flags & mrk::TF_BTREE) {
    uint64_t d = 0, least = ~0ull;
    for (uint32_t k = 0; k < P.n_terms && k < (uint32_t)MRK_MAX_AND_TERMS; ++k) d += P.t[k].docs, least = std::min<uint64_t>(least, P.t[k].docs);
    return (P.tree_flags & mrk::TF_MULTIAND) && P.n_terms ? least : d; // (an AND of keywords holds no more docs than its rarest one)
  }
  return P.t[0].docs;
}

// The batch's scan_bm queries (items_bm entries of kind 0, one whole window range each) in groups, and per group the items_bm
// entry of its first member (a group's members share the window range)
static void group_bm_items(const DevQuery* head, uint32_t n, const std::vector<DevQuery>& extra, const std::vector<DevItem>& items_bm, bool nib,
                           std::vector<BmGroup>& groups, std::vector<uint32_t>& group_item) {
  auto pass = [&](uint32_t p) -> const DevQuery& { return p < n ? head[p] : extra[p - n]; };
  auto tkey = [](const DevTerm& T) { // (bitmap, idf): one key = one tfidf table
    uint32_t idf;
    memcpy(&idf, &T.idf, 4);
    return std::make_pair(T.bm_off, idf);
  };
  std::vector<std::pair<uint64_t, uint32_t>> keys;
  for (const DevItem& it : items_bm)
    if (it.kind == 0) keys.push_back(tkey(pass(it.query).t[0])), keys.push_back(tkey(pass(it.query).t[1]));
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  std::vector<uint32_t> ent; // items_bm index of member i
  std::vector<BmMember> mem;
  std::vector<uint32_t> cls_rep; // per class: a member's entry
  for (uint32_t e = 0; e < items_bm.size(); ++e) {
    const DevItem& it = items_bm[e];
    if (it.kind != 0) continue;
    const DevQuery& P = pass(it.query);
    const uint32_t nw = std::min<uint32_t>(P.n_weights, 8u);
    BmMember x{};
    x.cls = ~0u;
    for (uint32_t c = 0; c < cls_rep.size() && x.cls == ~0u; ++c) { // same windows, same field-weight table
      const DevItem& r = items_bm[cls_rep[c]];
      const DevQuery& R = pass(r.query);
      if (r.blk_begin == it.blk_begin && r.blk_end == it.blk_end && std::min<uint32_t>(R.n_weights, 8u) == nw &&
          !memcmp(R.weights, P.weights, nw * sizeof(int32_t)))
        x.cls = c;
    }
    if (x.cls == ~0u) x.cls = (uint32_t)cls_rep.size(), cls_rep.push_back(e);
    for (int t = 0; t < 2; ++t) {
      x.key[t] = (uint64_t)(std::lower_bound(keys.begin(), keys.end(), tkey(P.t[t])) - keys.begin());
      x.bytes[t] = (uint64_t)(it.blk_end - it.blk_begin) * 256 + (uint64_t)P.t[t].nblocks * (nib ? 128 : 256);
    }
    ent.push_back(e), mem.push_back(x);
  }
  std::vector<uint32_t> order, sizes;
  plan_bm_groups(mem, order, sizes);
  groups.clear(), group_item.clear();
  size_t o = 0;
  for (uint32_t sz : sizes) {
    BmGroup g{};
    g.n = sz;
    g.per = WAVES / sz;
    uint64_t tab_key[BM_GROUP_TABS];
    for (uint32_t j = 0; j < sz; ++j) {
      const uint32_t i = order[o + j];
      g.q[j] = items_bm[ent[i]].query;
      for (uint32_t t = 0; t < 2; ++t) {
        uint32_t k = 0;
        while (k < g.ntab && tab_key[k] != mem[i].key[t]) ++k;
        if (k == g.ntab) tab_key[g.ntab] = mem[i].key[t], g.tab_src[g.ntab++] = j << 1 | t; // (<= 5: every member holds the seed)
        g.tab_idx |= k << (6 * j + 3 * t);
      }
    }
    groups.push_back(g);
    group_item.push_back(ent[order[o]]);
    o += sz;
  }
}

void mrk::place_bm_items(const DevQuery* head, uint32_t n, const std::vector<DevQuery>& extra, const BatchLayout& lay, bool nib, int mode,
                         BmPlacement& out) {
  const uint32_t n0 = (uint32_t)lay.n_items_kind[0];
  const DevItem* const it = lay.items.data() + lay.n_items_pk;
  out.disp.resize(n0);
  out.owner_class.clear(), out.owner_pass.clear();
  out.owner_keys = out.class_keys = 0;
  out.owner_bytes = out.class_bytes = 0;
  out.ran = out.mismatch = false;
  auto identity = [&]() {
    for (uint32_t i = 0; i < n0; ++i) out.disp[i] = i;
  };
  auto pass = [&](uint32_t p) -> const DevQuery& { return p < n ? head[p] : extra[p - n]; };
  // ---- owners: the ranges layout_batch cut (groups, or queries), their piece length and count.  Nothing below reads the
  // items themselves unless the section's order is not one of the two this function can index (see `tiers`)
  const bool grouped = !lay.groups.empty();
  const uint32_t n_own = (uint32_t)lay.bm_whole.size();
  typedef BmPlacement::Own Own;
  BmPlacement::Scratch& S = out.scratch; // (every list below lives there: a batch's next submit finds the buffers grown)
  std::vector<Own>& own = S.own;
  own.assign(n_own, Own{});
  std::vector<uint32_t>& live = S.live; // owners with items, ascending
  live.clear();
  uint64_t total = 0;
  uint32_t unit = ~0u;
  for (uint32_t o = 0; o < n_own; ++o) {
    Own& w = own[o];
    w.begin = lay.bm_whole[o].blk_begin, w.end = lay.bm_whole[o].blk_end, w.len = (uint32_t)std::max<uint64_t>(lay.bm_len[o], 1);
    w.items = w.end > w.begin ? (w.end - w.begin + w.len - 1) / w.len : 0;
    if (!grouped) out.owner_pass.push_back(lay.bm_whole[o].query);
    if (w.items) live.push_back(o), total += w.items, unit = std::min(unit, w.items);
  }
  out.owner_class.assign(n_own, 0);
  out.mismatch = mode != 0 && total != n0; // (the ranges and the section disagree: never from layout_batch; the caller fails the submit)
  if (mode == 0 || live.size() < 2 || out.mismatch) return identity();
  // ---- keywords: dense ids of the (bitmap, idf) keys, a key's bytes as group_bm_items charges them (the largest of its holders')
  auto tkey = [](const DevTerm& T) {
    uint32_t idf;
    memcpy(&idf, &T.idf, 4);
    return std::make_pair(T.bm_off, idf);
  };
  auto n_terms_of = [&](uint32_t o) { return grouped ? lay.groups[o].ntab : 2u; };
  auto owner_term = [&](uint32_t o, uint32_t j) -> const DevTerm& { // keyword j of owner o: a group's table j, a query's keyword j
    if (!grouped) return pass(out.owner_pass[o]).t[j];
    const BmGroup& G = lay.groups[o];
    return pass(G.q[G.tab_src[j] >> 1]).t[G.tab_src[j] & 1u];
  };
  uint32_t n_terms = 0;
  for (uint32_t o : live) n_terms += n_terms_of(o);
  uint32_t hmask = 63;
  while (hmask < 4 * n_terms) hmask = 2 * hmask + 1;
  std::vector<uint32_t>& slot = S.slot; // open addressing: a slot names its key's id
  slot.assign(hmask + 1, ~0u);
  std::vector<std::pair<uint64_t, uint32_t>>& keys = S.keys;
  std::vector<uint64_t>& kb = S.kb;
  keys.clear(), kb.clear();
  for (uint32_t o : live) {
    Own& w = own[o];
    for (uint32_t j = 0; j < n_terms_of(o); ++j) {
      const DevTerm& T = owner_term(o, j);
      const std::pair<uint64_t, uint32_t> key = tkey(T);
      uint32_t h = (uint32_t)((key.first * 0x9E3779B97F4A7C15ull + key.second * 0xC2B2AE3D27D4EB4Full) >> 40) & hmask;
      while (slot[h] != ~0u && keys[slot[h]] != key) h = (h + 1) & hmask;
      if (slot[h] == ~0u) slot[h] = (uint32_t)keys.size(), keys.push_back(key), kb.push_back(0);
      const uint32_t k = slot[h];
      kb[k] = std::max(kb[k], (uint64_t)(w.end - w.begin) * 256 + (uint64_t)T.nblocks * (nib ? 128 : 256));
      bool have = false;
      for (uint32_t x = 0; x < w.nkeys; ++x) have = have || w.key[x] == k;
      if (!have) w.key[w.nkeys++] = k;
    }
  }
  const uint32_t nk = (uint32_t)keys.size();
  for (uint32_t o : live) {
    for (uint32_t x = 0; x < own[o].nkeys; ++x) own[o].bytes += kb[own[o].key[x]];
    out.owner_keys += own[o].nkeys, out.owner_bytes += own[o].bytes;
  }
  // ---- classes.  The cap leaves two units of slack (a unit = the smallest owner's items, a lone query's): with one, the
  // classes fill to the brim and hardly a move is possible (the benchmark's sets: 0.72-0.78 of the owners' bytes; with two,
  // 0.66-0.71).  What the slack costs is affinity in the launch's tail only, since a class that runs out hands its slots on:
  // under 4 % of those sets' items.
  const uint32_t n_cls = mode == 1 ? PLACE_CLASSES : 1u;
  std::vector<uint16_t>& cnt = S.cnt; // holders of key k in class c
  cnt.assign((size_t)n_cls * nk, 0);
  uint64_t load[PLACE_CLASSES] = {};
  std::vector<uint8_t>& cls = out.owner_class;
  auto add_cost = [&](uint32_t o, uint32_t c) {
    uint64_t b = 0;
    for (uint32_t x = 0; x < own[o].nkeys; ++x) b += cnt[(size_t)c * nk + own[o].key[x]] ? 0 : kb[own[o].key[x]];
    return b;
  };
  auto put = [&](uint32_t o, uint32_t c, int d) {
    for (uint32_t x = 0; x < own[o].nkeys; ++x) cnt[(size_t)c * nk + own[o].key[x]] += d;
    load[c] += (int64_t)d * own[o].items;
    if (d > 0) cls[o] = (uint8_t)c;
  };
  if (n_cls > 1) {
    const uint64_t cap = (total + n_cls - 1) / n_cls + 2 * (uint64_t)unit;
    std::vector<uint32_t>& by_load = S.by_load;
    by_load.assign(live.begin(), live.end());
    std::sort(by_load.begin(), by_load.end(), [&](uint32_t a, uint32_t b) {
      if (own[a].items != own[b].items) return own[a].items > own[b].items;
      if (own[a].bytes != own[b].bytes) return own[a].bytes > own[b].bytes;
      return a < b;
    });
    for (uint32_t o : by_load) {
      uint32_t best = ~0u, lightest = 0;
      uint64_t best_cost = 0;
      for (uint32_t c = 0; c < n_cls; ++c) {
        if (load[c] < load[lightest]) lightest = c;
        if (load[c] + own[o].items > cap) continue;
        const uint64_t cost = add_cost(o, c);
        if (best == ~0u || cost < best_cost || (cost == best_cost && load[c] < load[best])) best = c, best_cost = cost;
      }
      put(o, best == ~0u ? lightest : best, 1);
    }
    for (int sweep = 0; sweep < 8; ++sweep) { // single moves that lower the sum of the classes' bytes (in practice two or three sweeps find any)
      bool moved = false;
      for (uint32_t o : live) {
        const uint32_t c0 = cls[o];
        uint64_t freed = 0;
        for (uint32_t x = 0; x < own[o].nkeys; ++x) freed += cnt[(size_t)c0 * nk + own[o].key[x]] == 1 ? kb[own[o].key[x]] : 0;
        uint32_t best = ~0u;
        uint64_t best_cost = 0;
        for (uint32_t c = 0; c < n_cls && freed; ++c) {
          if (c == c0 || load[c] + own[o].items > cap) continue;
          const uint64_t cost = add_cost(o, c);
          if (cost >= freed) continue;
          if (best == ~0u || cost < best_cost || (cost == best_cost && load[c] < load[best])) best = c, best_cost = cost;
        }
        if (best == ~0u) continue;
        put(o, c0, -1), put(o, best, 1);
        moved = true;
      }
      if (!moved) break;
    }
  } else
    for (uint32_t o : live) put(o, 0, 1);
  for (uint32_t c = 0; c < n_cls; ++c)
    for (uint32_t k = 0; k < nk; ++k)
      if (cnt[(size_t)c * nk + k]) ++out.class_keys, out.class_bytes += kb[k];
  // ---- where piece k of owner o sits in the section.  Query-major: behind the owners before it.  Piece-major: the pieces
  // k of the owners that have one, in owner order; between two of the owners' distinct piece counts ("tiers": one per group
  // size and window range) the same owners are alive, so the index is linear in k there.  More tiers than fit the table
  // (queries with window ranges of their own): the items are read once instead.
  constexpr uint32_t MAX_TIERS = 8;
  std::vector<uint32_t>& first = S.first;
  first.assign(n_own + 1, 0);
  for (uint32_t o = 0; o < n_own; ++o) first[o + 1] = first[o] + own[o].items;
  uint32_t tier_end[MAX_TIERS], tier_base[MAX_TIERS], tier_alive[MAX_TIERS], n_tiers = 0;
  std::vector<uint32_t>& rank = S.rank;
  bool tiers = lay.bm_piece_major;
  if (tiers) {
    std::vector<uint32_t>& counts = S.counts;
    counts.clear();
    for (uint32_t o : live) counts.push_back(own[o].items);
    std::sort(counts.begin(), counts.end());
    counts.erase(std::unique(counts.begin(), counts.end()), counts.end());
    tiers = counts.size() <= MAX_TIERS;
    if (tiers) {
      n_tiers = (uint32_t)counts.size();
      rank.assign((size_t)n_tiers * n_own, 0);
      uint32_t base = 0, from = 0;
      for (uint32_t j = 0; j < n_tiers; ++j) {
        uint32_t alive = 0;
        for (uint32_t o = 0; o < n_own; ++o)
          if (own[o].items >= counts[j]) rank[(size_t)j * n_own + o] = alive++;
        tier_end[j] = counts[j], tier_base[j] = base, tier_alive[j] = alive;
        base += (counts[j] - from) * alive, from = counts[j];
      }
    }
  }
  std::vector<uint32_t>& by_own = S.by_own;
  if (lay.bm_piece_major && !tiers) {
    by_own.resize(n0);
    std::vector<uint32_t>&fill = S.fill, &own_of = S.own_of;
    fill.assign(first.begin(), first.end() - 1);
    if (!grouped) {
      own_of.assign((size_t)n + extra.size(), 0);
      for (uint32_t o = 0; o < n_own; ++o) own_of[out.owner_pass[o]] = o;
    }
    for (uint32_t i = 0; i < n0; ++i) by_own[fill[grouped ? it[i].query : own_of[it[i].query]]++] = i;
  }
  // ---- inside a class: ascending blk_begin, then owner (begin by begin, the class's owners in order).  The s-th item of class
  // x runs in slot n_cls s + x as long as every class has an s-th item; what is left then goes to `rest`, class by class
  uint32_t least = ~0u, rest_first[PLACE_CLASSES + 1] = {};
  for (uint32_t c = 0; c < n_cls; ++c) least = std::min<uint64_t>(least, load[c]);
  for (uint32_t c = 0; c < n_cls; ++c) rest_first[c + 1] = rest_first[c] + (uint32_t)load[c] - least;
  std::vector<uint32_t>& rest = S.rest;
  rest.resize(rest_first[n_cls]);
  typedef BmPlacement::Cur Cur;
  auto locate = [&](Cur& m) { // the place of piece m.k of owner m.o
    if (tiers) {
      while (m.k >= tier_end[m.tier]) ++m.tier;
      m.idx = tier_base[m.tier] + (m.k - (m.tier ? tier_end[m.tier - 1] : 0)) * tier_alive[m.tier] + rank[(size_t)m.tier * n_own + m.o];
      m.step = tier_alive[m.tier], m.run = tier_end[m.tier] - m.k;
    } else if (lay.bm_piece_major)
      m.idx = by_own[first[m.o] + m.k], m.step = 0, m.run = 1;
    else
      m.idx = first[m.o] + m.k, m.step = 1, m.run = ~0u;
  };
  std::vector<Cur>& mem = S.mem;
  uint32_t* const disp = out.disp.data();
  for (uint32_t c = 0; c < n_cls; ++c) {
    mem.clear();
    for (uint32_t o : live)
      if (cls[o] == c) {
        Cur m{own[o].begin, own[o].len, own[o].items, 0, 0, 0, o, 0, 0};
        locate(m);
        mem.push_back(m);
      }
    uint32_t s = 0;
    const uint32_t want = (uint32_t)load[c];
    uint32_t* const own_slots = disp + c;
    uint32_t* const spill = rest.data() + rest_first[c];
    for (uint64_t x = 0, nx; s < want; x = nx) { // every owner whose next piece begins at x (the least begin left), then the next begin
      nx = ~0ull;
      for (Cur& m : mem) {
        if (!m.left) continue;
        if (m.next <= x) {
          if (s < least)
            own_slots[(size_t)s * n_cls] = m.idx;
          else
            spill[s - least] = m.idx;
          ++s, ++m.k, --m.left, m.next += m.len, m.idx += m.step;
          if (!--m.run && m.left) locate(m);
          if (!m.left) continue;
        }
        nx = std::min<uint64_t>(nx, m.next);
      }
    }
  }
  // ---- the tail: a class that has run out hands its slots to the class with the most items left
  uint32_t next[PLACE_CLASSES];
  for (uint32_t c = 0; c < n_cls; ++c) next[c] = rest_first[c];
  for (uint32_t i = least * n_cls; i < n0; ++i) {
    uint32_t c = i % n_cls;
    if (next[c] == rest_first[c + 1])
      for (uint32_t d = 0; d < n_cls; ++d)
        if (rest_first[d + 1] - next[d] > rest_first[c + 1] - next[c]) c = d;
    disp[i] = rest[next[c]++];
  }
  out.ran = true;
}

// Walks the pieces 0, 1, ... of ranges 0 .. n_ranges (piece(r, k) emits piece k of range r, or returns false past the range's
// end): query-major, a range's pieces back to back, or piece-major, the k-th piece of every range, then the (k+1)-th ...
template <class Piece>
static void for_pieces(size_t n_ranges, bool piece_major, Piece piece) {
  if (!piece_major) {
    for (size_t r = 0; r < n_ranges; ++r)
      for (uint64_t k = 0; piece(r, k); ++k) {}
    return;
  }
  for (uint64_t k = 0;; ++k) {
    bool any = false;
    for (size_t r = 0; r < n_ranges; ++r) any = piece(r, k) || any;
    if (!any) break;
  }
}

// piece k of `whole` cut into pieces of `len`, appended to `out`; false past its end
static bool cut_piece(const DevItem& whole, uint64_t len, uint64_t k, std::vector<DevItem>& out) {
  const uint64_t x = whole.blk_begin + k * len;
  if (x >= whole.blk_end) return false;
  DevItem it = whole;
  it.blk_begin = (uint32_t)x;
  it.blk_end = (uint32_t)std::min<uint64_t>(whole.blk_end, x + len);
  out.push_back(it);
  return true;
}

void mrk::layout_batch(DevQuery* head, uint32_t n, BatchPlan& plan, bool use_packed, bool nibble_plane, const LayoutKnobs& knobs, BatchLayout& out) {
  std::vector<DevQuery>& extra = plan.extra;
  const std::vector<DevItem>& items_bm = plan.items_bm;
  const bool any_prox = plan.any_prox;
  out = BatchLayout{};
  std::vector<DevItem>& items = out.items;
  items.swap(plan.items);
  // A small batch (one-eighth shards, selective keywords, a lone query): the planner cuts a driver doclist into ~item_bytes
  // pieces whatever the batch holds, and 280 workgroups that each walk 70 blocks per wave one after the other leave the chip
  // idle for 0.1 ms.  Cut the block ranges finer until the launch has pk_min_items work items (never under one block per wave).
  // A launch on the lean instance (p2_max_blocks): a wave there is a chain of dependent round trips per driver block, and the launch
  // lasts as long as its longest waves, so no item keeps more than the cap's blocks however many items the launch already has.
  // The piece length is the smaller of the two rules', a multiple of T0_BLOCKS.
  const bool few = items.size() < (size_t)knobs.pk_min_items;
  if (use_packed && !items.empty() && (few || knobs.p2_max_blocks > 0)) {
    uint64_t total_blocks = 0;
    for (const DevItem& it : items) total_blocks += it.blk_end - it.blk_begin;
    uint64_t per = ~0ull;
    if (few) {
      per = (total_blocks + (uint64_t)knobs.pk_min_items - 1) / (uint64_t)knobs.pk_min_items;
      per = std::max<uint64_t>(T0_BLOCKS, (per + T0_BLOCKS - 1) / T0_BLOCKS * T0_BLOCKS);
    }
    if (knobs.p2_max_blocks > 0) per = std::min<uint64_t>(per, std::max<uint64_t>(T0_BLOCKS, (uint64_t)knobs.p2_max_blocks / T0_BLOCKS * T0_BLOCKS));
    std::vector<DevItem> cut;
    cut.reserve(items.size() + (size_t)(total_blocks / per) + 1);
    std::vector<uint32_t> per_pass((size_t)n + extra.size(), 0);
    for_pieces(items.size(), false, [&](size_t r, uint64_t k) {
      if (!cut_piece(items[r], per, k, cut)) return false;
      if (items[r].query < per_pass.size()) ++per_pass[items[r].query];
      return true;
    });
    items.swap(cut);
    // (the counts feed the match-queue sizing below; the VLB path's per-query list ranges are not built from a packed plan)
    for (uint32_t i = 0; i < n; ++i)
      if (per_pass[i]) head[i].n_items = per_pass[i];
    for (size_t e = 0; e < extra.size(); ++e)
      if (per_pass[n + e]) extra[e].n_items = per_pass[n + e];
  }
  // ... and in piece-major order, for the reason given at the window-range items below: concurrent workgroups should belong
  // to different queries (the planner emits a query's items back to back; only the VLB path needs them that way)
  // (not for batches whose matches travel through the match queue to the hit pass: config 3 measured 6.6 ms query-major, 7.1 ms
  // interleaved -- the rank kernel likes a query's chunks in rowid order)
  if (use_packed && items.size() > 1 && (knobs.item_order & 1) && (!any_prox || (knobs.item_order & 8))) {
    std::vector<size_t> run_begin, run_end; // runs of items of one pass: its ranges, their pieces the items
    for (size_t i = 0; i < items.size();) {
      size_t j = i + 1;
      while (j < items.size() && items[j].query == items[i].query) ++j;
      run_begin.push_back(i), run_end.push_back(j);
      i = j;
    }
    std::vector<DevItem> rr;
    rr.reserve(items.size());
    for_pieces(run_begin.size(), true, [&](size_t r, uint64_t k) {
      if (run_begin[r] + k >= run_end[r]) return false;
      rr.push_back(items[run_begin[r] + k]);
      return true;
    });
    items.swap(rr);
  }
  out.t_block_items = std::chrono::steady_clock::now();
  out.n_items_pk = items.size();
  // window-range work items (two-bitmap AND kernel, then the window-driven tree kernel) ride behind the block work
  // items; each kind's whole-range entries are cut once the batch's total is known (a wave's fixed costs -- tables, final
  // publish, atomics on the query's counters -- want long runs of windows)
  for (uint32_t kind = 0; kind < 2; ++kind) {
    uint64_t total_win = 0;
    for (const DevItem& it : items_bm)
      if (it.kind == kind) total_win += it.blk_end - it.blk_begin;
    if (!total_win) continue;
    const uint64_t unit = 4 * WAVES; // one burst per wave
    uint64_t wpi = (total_win / (uint64_t)(kind == 0 ? knobs.bm_target_items : knobs.bt_target_items) / unit) * unit;
    wpi = std::min<uint64_t>(std::max<uint64_t>(wpi, kind == 0 ? (uint64_t)knobs.bm_min_windows / unit * unit : 4 * unit), 4096); // (short runs: a wave's fixed costs show -- 12.5 M docs, 8192 items: 0.55 vs 0.47 ms)
    std::vector<DevItem> whole; // the ranges to cut ...
    std::vector<uint64_t> len;  // ... and each one's piece length
    if (kind == 0 && knobs.bm_group && (knobs.item_order & 2)) {
      // Queries that share a keyword run in one workgroup, a wave (or two) per member over the same windows: the shared
      // keyword's bitmap words and tf / field lines are then fetched once per CU instead of once per query
      std::vector<uint32_t> group_item; // per group its first member's whole-range entry in items_bm
      group_bm_items(head, n, extra, items_bm, nibble_plane, out.groups, group_item);
      for (uint32_t g = 0; g < out.groups.size(); ++g) {
        ++out.n_bm_groups[out.groups[g].n - 1];
        whole.push_back(items_bm[group_item[g]]);
        whole.back().query = g;
        len.push_back(wpi * out.groups[g].per / WAVES); // a wave walks wpi / WAVES windows, as in the ungrouped layout
      }
    } else
      for (const DevItem& it : items_bm)
        if (it.kind == kind) whole.push_back(it), len.push_back(wpi);
    // Piece-major order: the k-th piece of every query, then the (k+1)-th ...  Workgroups that run at the same time then
    // belong to DIFFERENT queries.  Query-major order put a query's 20-50 workgroups on the chip together, all of them adding
    // to the one candidate counter, the same few histogram bins and the one threshold word of that query: device-scope
    // atomics on one address serialize at the memory side (~70 ns each), about 0.1 ms per query whatever the shard size --
    // hidden behind 100 M docs, the whole launch at 12.5 M (12288 work items: 0.85 ms; 4096: 0.39 ms, same bytes).
    // Query-major: experiments, and trees that feed the match queue (see the block items above).
    const bool piece_major = (knobs.item_order & (kind == 0 ? 2 : 4)) && !(kind == 1 && any_prox && !(knobs.item_order & 8));
    const size_t before = items.size();
    for_pieces(whole.size(), piece_major, [&](size_t r, uint64_t k) { return cut_piece(whole[r], len[r], k, items); });
    if (kind == 0) out.bm_piece_major = piece_major, out.bm_whole.swap(whole), out.bm_len.swap(len);
    out.n_items_kind[kind] = items.size() - before;
  }
  for (const DevItem& it : items_bm) // the generic evaluator's candidates: block ranges, cut by the planner
    if (it.kind == 2) items.push_back(it), ++out.n_items_kind[2];
  // match queues: a pass hands over at most one entry per doc it can match, plus one partial chunk per wave of its items
  uint64_t (&mq_chunks)[3] = out.mq_chunks;
  if (use_packed && any_prox) {
    bool bt_feeds[3] = {false, false, false};
    auto account = [&](const DevQuery& P) {
      bool fat = false;
      if (!P.n_items || !pass_queues_matches(P, fat)) return;
      const bool bt = (P.tree_flags & mrk::TF_BTREE) != 0;
      mq_chunks[queue_of(P, fat)] += pass_max_matches(P) / 64 + (bt ? 0 : 4ull * (mrk::MQ_BATCH + 1) * P.n_items) + 1;
      bt_feeds[queue_of(P, fat)] = bt_feeds[queue_of(P, fat)] || bt;
    };
    for (uint32_t i = 0; i < n; ++i) account(head[i]);
    for (const DevQuery& P : extra) account(P);
    for (int i = 0; i < 2; ++i) // per wave one partial chunk + the unused rest of a reservation (its work items were only cut just now)
      if (bt_feeds[i]) mq_chunks[i] += 4ull * (mrk::MQ_BATCH + 1) * out.n_items_kind[1];
    for (int i = 0; i < 3; ++i) mq_chunks[i] = std::min<uint64_t>(mq_chunks[i], (uint64_t)knobs.mq_max_chunks);
  }
}
