// mrk_host_int.h -- host-side objects shared by mrk_host.cpp (segments, batches, C-ABI) and mrk_plan.cpp (query planner, launch layout).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <chrono>
#include <utility>
#include <vector>

#include "mrk_dev.h"
#include "mrk_kgroup.h"

int mrk_fail(int code, const char* fmt, ...);

using mrk::DevItem;
using mrk::DevQuery;
using mrk::DevSegment;
using mrk::DevTerm;

struct mrk_worker; // the context's submission thread (mrk_host.cpp)
struct mrk_comm;   // the context's RCCL communicator for the shard exchange (mrk_comm.cpp)

struct mrk_ctx {
  std::atomic<int> n_segments{0}, n_batches{0}; // alive through the C-ABI: mrk_ctx_destroy refuses while any is
  mrk_worker* worker = nullptr;
  mrk_comm* comm = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t merge_stream = nullptr; // mrk_topk_merge: never queued behind the scans of a following batch
  hipEvent_t merge_done[MRK_MERGE_SLOTS] = {};
  bool merge_used[MRK_MERGE_SLOTS] = {};
  uint64_t* gmerge = nullptr;     // group- and aggregate-row merges (mrk_topk_merge_grows* / _arows*): the scratch arena of their tables, one per query of a call, ...
  size_t gmerge_words = 0;        // ... grown on demand, cleared on merge_stream in front of every merge
  int64_t item_bytes = 128 << 10; // target doclist bytes per work item
  int path = 0;                   // 0 = packed doclists when the segment has them, 1 = VLB (.spd) direct, 2 = packed only
  int pack = 1;                   // build packed doclists at segment load
  int bitmap_inv = 64;            // terms in >= 1/bitmap_inv of the docs also get a bitmap (0 = never)
  int attr_seq = 1;               // keywords with a bitmap also get their tf / field bytes in slot order (what the bitmap kernel gathers from)
  int bm_wmax = 1;                // keywords with a bitmap also get a 4-bit largest-tf class per bitmap word: the bitmap kernel drops match words whose best possible weight lies behind the threshold (0 = no plane, the kernel as before)
  int attr_nibbles = 0;           // also build the one-byte tf/field plane the bitmap kernel can gather from (<= 4 fields)
  int bm_target_items = 1 << 20;  // two-bitmap AND kernel: cap of the work items per launch ...
  int bm_min_windows = 256;       // ... and the least windows per work item (a wave's fixed costs show on short runs; 128 until the items were dispatched in window order)
  int bm_place = 2;               // ... and the order its work items are dispatched in: 2 = window order; 1 = owners that share keywords on one XCD, each XCD in window order (slower: DESIGN section 6); 0 = as laid out
  int bm_place_min_items = 16384; // ... from this many work items per launch on (a shorter launch is over before the order pays for its host time)
  int bm_group = 1;               // two-bitmap AND kernel: queries that share a keyword run in one workgroup, a wave per member (0 = a workgroup per query)
  int pair_scan = 1;              // block-scan launches of plain one- and two-keyword queries take the lean instance (mrk_scan_p2.hip); 0 = the generic one
  int pk_min_items = 2048;        // block-scan kernel: a batch with fewer work items has its block ranges cut finer (>= one block per wave)
  int p2_max_blocks = 4;          // ... and a launch on the lean instance keeps no work item longer than this many driver blocks (a multiple of the 4 waves; 0 = no cap; pk_min_items = 1 turns the whole recut off, this cap included)
  int exchange_part = 1;          // mrk_shard_exchange partitions the merge by query (all-to-all of row slices); 0 = all-gather, every rank merges everything
  int prox_prune = 1;             // proximity rankers: matches whose weight upper bound cannot reach the top K skip the hit pass (counted, not ranked)
  int exchange_self_rccl = 0;     // one rank: still send the rows to itself through RCCL (rehearsal of the collective path)
  int item_order = 7;             // work items of different queries interleaved (piece-major): 1 = block scan, 2 = bitmap AND, 4 = bitmap trees; 0 = query-major
  int bt_target_items = 6144;     // ... and the tree kernel over bitmap words
  int prox_bound_keywords = 0;    // 1: equal positions of different keywords sort by query position in this context's indexes (see mrk.h) -- the tighter weight bound is sound
  int bt_phrase = 1;              // root PHRASE / PROXIMITY of common words: the AND of the words runs on bitmap words too (0 = block walk)
  int bt_cover_inv = 1024;        // trees whose candidate cover holds >= 1/bt_cover_inv of the docs run on bitmap words (0 = never; 32 until the step grew to 8192 rowids: config 3 5.4 -> 4.8 ms)
  int gen_lane_hits = 256;        // generic evaluator: hits (16 B) of per-lane list memory, GEN_GRID * 256 lanes
  int gen_spill_mb = 1024;        // ... and the shared area for lists beyond a lane's slice (exhausted: the query fails loudly)
  int mq_max_chunks = 1 << 22;    // cap of a batch's match queue, in 64-entry chunks of 1792 B (a fuller queue flags its queries: rerun alone)
};

struct HostTerm {
  uint64_t doclist_off = 0, doclist_len = 0;
  uint64_t packed_bytes = 0;
  uint32_t blk_first = 0, nblocks = 0, docs = 0, hits = 0;
  uint32_t exc_first = 0, exc_n = 0;
  uint32_t last_rowid = 0; // rowid of the term's last doc (packed segments)
  uint64_t bm_off = ~0ull, dir_off = ~0ull; // word offsets of the term's bitmap / rank directory, ~0 = none
};

struct mrk_segment {
  mrk_ctx* ctx = nullptr;
  DevSegment dev{};
  std::vector<HostTerm> terms;
  uint64_t total_docs = 0;
  uint32_t n_fields = 0;
  uint64_t device_bytes = 0;
  void* d_spd = nullptr;
  void* d_spp = nullptr;
  void* d_blk_base = nullptr;
  void* d_blk_off = nullptr;
  void* d_blk_hit = nullptr;
  bool has_packed = false;
  void* d_pk_base = nullptr;
  void* d_pk_doff = nullptr;
  void* d_pk_w = nullptr;
  void* d_pk_delta = nullptr;
  void* d_pk_attr = nullptr;
  void* d_pk_exc = nullptr;
  void* d_pk_hit = nullptr;
  void* d_pk_hbase = nullptr;
  void* d_pk_attr1 = nullptr;
  void* d_pk_attr2 = nullptr;
  void* d_pk_fmask = nullptr;
  bool wide = false; // packed in the layout for 9-32 fields (pk_fmask): the scan kernel's WIDE instances, no bitmap-driven kernels
  void* d_dead = nullptr;
  void* d_attrs = nullptr; // .spa rows (mrk_segment_set_attrs)
  void* d_blobs = nullptr; // blob pool (mrk_segment_set_blobs)
  uint32_t n_blob_attrs = 0;
  uint64_t attr_rows = 0;
  // sorted queries (mrk_query.sort): the rows are kept on the host too -- the planner takes the range of a sort column from them
  // (one pass per locator, cached here until mrk_segment_set_attrs is called again) and mrk_batch_result reads mrk_result.sort_key
  std::vector<uint32_t> h_attrs;
  struct SortRange {
    int32_t bit_offset, bit_count, is_float;
    uint32_t lo, hi; // least / largest mapped key of the DESCENDING order (mrk_sortkey.h); lo > hi: no rows
    bool has_nan;
    uint64_t lo64 = 0, hi64 = 0; // a 64-bit column (is_float == MRK_SORTKEY_INT64, mrk_query.order): the same, of order_map_i64
  };
  // (written by plan_query through a const segment: planning runs on the context's ONE submission thread; with MRK_INLINE_HIP=1 the
  // caller must not submit sorted queries against one segment from two threads at once)
  mutable std::vector<SortRange> sort_ranges;
  void* d_bm = nullptr;
  void* d_bm_dir = nullptr;
  void* d_bm_wmax = nullptr;
  bool bitmaps_on = false; // packed with bitmap_inv != 0: every keyword dense enough for the block scan's direct map carries a bitmap
};

// mrk_comm.cpp (run on the submission thread)
int mrk_comm_unique_id_impl(uint8_t* id_out);
int mrk_comm_init_impl(mrk_ctx* ctx, const uint8_t* id_bytes, int n_ranks, int rank);
void mrk_comm_destroy_impl(mrk_ctx* ctx);
int mrk_comm_allreduce_i64_impl(mrk_ctx* ctx, int64_t* values, uint64_t n);
int mrk_comm_exchange_impl(mrk_ctx* ctx, const uint64_t* rows, uint32_t n_queries, uint32_t row_words, hipEvent_t after, uint32_t slot, const uint64_t** rows_all_out,
                           hipEvent_t* gathered_event_out);
int mrk_comm_ranks(const mrk_ctx* ctx);
int mrk_comm_rank(const mrk_ctx* ctx);
void mrk_shard_slice_impl(uint32_t n_queries, int n_ranks, int rank, uint32_t* per_out, uint32_t* first_out, uint32_t* count_out);
bool mrk_comm_can_partition(mrk_ctx* ctx);
int mrk_comm_exchange_part_impl(mrk_ctx* ctx, const uint64_t* rows, uint32_t n_queries, uint32_t row_words, hipEvent_t after, uint32_t slot, const uint64_t** recv_out,
                                hipEvent_t* gathered_event_out, uint32_t* per_out, uint32_t* first_out, uint32_t* count_out);
int mrk_comm_flags_begin(mrk_ctx* ctx, uint32_t slot, uint32_t** flags_dev_out);
int mrk_comm_flags_finish(mrk_ctx* ctx, uint32_t slot);
int mrk_comm_flags_read(mrk_ctx* ctx, uint32_t slot, uint32_t* rerun_any, uint32_t* declined_any);
hipEvent_t mrk_comm_rows_ready_event(mrk_ctx* ctx);

namespace mrk {

// What the planning loop of one batch accumulates: plan_query appends a query's passes, work items and byte counts to it, and
// layout_batch turns it into the launch's item array.
struct BatchPlan {
  std::vector<DevQuery> extra;     // passes beyond a query's head pass; pass index = n_queries + position
  std::vector<DevItem> items;      // block-scan work items, a query's back to back
  std::vector<DevItem> items_bm;   // one whole window range per scan_bm (kind 0) / scan_bt (kind 1) pass; the generic evaluator's block items (kind 2), already cut
  std::vector<GenProg> gen_progs;  // programs of the generic evaluator (DevQuery::gen_prog indexes it)
  uint64_t algo_bytes = 0, dev_bytes = 0, cand_total = 0;
  uint64_t sort_total = 0;         // 16-byte candidate slots of the batch's sorted queries (mrk_query.sort); 0 = it holds none
  uint64_t group_total = 0;        // u64 words of the batch's group tables (mrk_group, mrk_kgroup.h); 0 = it holds no grouped query
  bool any_prox = false, any_tree = false;
  // a declined query runs no device work: what it appended is taken back (the byte counts and flags stay as plan_query left them)
  struct Mark { size_t extra, items, items_bm, gen_progs; };
  Mark mark() const { return Mark{extra.size(), items.size(), items_bm.size(), gen_progs.size()}; }
  void rewind(const Mark& m) { extra.resize(m.extra), items.resize(m.items), items_bm.resize(m.items_bm), gen_progs.resize(m.gen_progs); }
};

// Plans one query of a batch: validates it, builds the reference-shaped evaluation tree, computes IDFs, pruning
// histogram geometry and candidate capacity, and emits the query's passes and work items into `plan`.  Returns MRK_OK, or
// MRK_E_UNSUPPORTED / MRK_E_INVAL with the message set.  dq = the query's head pass (index qi); further passes go to
// plan.extra and get pass indices n_queries + position.  group: the query's mrk_group (mrk_batch_submit_grouped) or NULL -- a grouped
// query gets a table of plan.group_total's arena instead of a candidate list (DevQuery::grp_*; all zero for every other query).
// aggrs: the grouped query's mrk_aggrs (mrk_batch_submit_aggr) or NULL -- its table gets one accumulator plane per aggregate behind the
// counts (DevQuery::grp_naggr, grp_aggr_*, grp_order_aggr); a query without them plans word for word as without the argument.
// mva: the grouped query's mrk_group_mva (mrk_batch_submit_mva) or NULL -- the group's values are a multi-value attribute's
// (DevQuery::grp_pad, the MVA word; grp_item / grp_shift / grp_bits 0 / 0 / 32); the table, the routing and the rerun are a group's.
int plan_query(const mrk_segment* seg, const mrk_query& q, int64_t item_bytes, bool use_packed, DevQuery& dq, uint32_t n_queries, uint32_t qi,
               BatchPlan& plan, uint32_t rowid_max = 0xFFFFFFFFu, const mrk_group* group = nullptr, const mrk_aggrs* aggrs = nullptr,
               const mrk_group_mva* mva = nullptr);

// Groups of a batch's scan_bm queries for the grouped bitmap kernel ("bm_group", mrk_batch_submit).  A member names its two
// keywords (key: bitmap offset + idf bits, so that members sharing a key share its tfidf table too), the bytes a walk of each
// costs, and a class: only members of one class may share a group (same window range and field weights).  Deterministic
// greedy, per class: seed a group with the key held by the most members left (ties: the smaller key), then add, up to
// BM_GROUP_MAX, the holder of the seed that adds the fewest bytes of keys new to the group (ties: the lower index).  Members
// whose keys no other member left holds stay alone.  A key's bytes are taken per class (they depend on the window range).
// Per-key holder lists and counts: about O(members + groups x keys).  Out: the members, group by group, and each group's size.
struct BmMember {
  uint64_t key[2];
  uint64_t bytes[2];
  uint32_t cls;
};
void plan_bm_groups(const std::vector<BmMember>& m, std::vector<uint32_t>& order, std::vector<uint32_t>& sizes);

// mirrors scan_pk_kernel: matches of these passes leave through the match queue (state rankers over more than one
// keyword, whole-query PHRASE); `fat` = the queue whose consumer carries the word state machines
bool pass_queues_matches(const DevQuery& P, bool& fat);
int queue_of(const DevQuery& P, bool fat);
// upper bound of the docs a pass can match: its driver's docs; the common docs for the two-bitmap AND; any keyword's docs for
// a tree evaluated on bitmap words
uint64_t pass_max_matches(const DevQuery& P);

// The launch layout of a planned batch on the packed path (host arithmetic only): block ranges cut finer for small batches,
// the whole window ranges of scan_bm / scan_bt cut into pieces, each section in query-major or piece-major order, scan_bm
// queries that share a keyword put in groups, the match queues sized.
struct LayoutKnobs { // the context's settings of the same names
  int pk_min_items, item_order, bm_target_items, bm_min_windows, bt_target_items, bm_group, mq_max_chunks;
  int p2_max_blocks; // longest block-scan item, in driver blocks (0 = no cap): mrk_batch_submit sets it for launches on the lean instance
};
struct BatchLayout {
  std::vector<DevItem> items;       // launch order: block-scan items, then kind 0 (scan_bm), kind 1 (scan_bt), kind 2 (generic evaluator)
  size_t n_items_pk = 0;            // ... the first section's length
  size_t n_items_kind[3] = {0, 0, 0}; // ... and the others'
  std::vector<BmGroup> groups;      // grouped scan_bm: a kind-0 item's `query` indexes it (empty: it is a pass index)
  uint32_t n_bm_groups[BM_GROUP_MAX] = {}; // groups of 1 .. BM_GROUP_MAX members
  std::vector<DevItem> bm_whole;    // the whole window ranges the kind-0 section was cut from, one per group (per query where none were formed) ...
  std::vector<uint64_t> bm_len;     // ... each one's piece length ...
  bool bm_piece_major = false;      // ... and the order of the pieces (place_bm_items finds an owner's k-th piece by these, without a pass over the items)
  uint64_t mq_chunks[3] = {0, 0, 0}; // chunks of each match queue (0 = unused)
  std::chrono::steady_clock::time_point t_block_items; // when the block-scan section was in order (mrk_batch_stats::plan_ms ends there)
};
// head[0 .. n) = the queries' head passes; takes plan.items, and writes the piece counts of the passes it cut to their n_items
// (head and plan.extra).  nibble_plane: the segment has the one-byte tf/field plane (it halves what a keyword's walk costs a group).
void layout_batch(DevQuery* head, uint32_t n, BatchPlan& plan, bool use_packed, bool nibble_plane, const LayoutKnobs& knobs, BatchLayout& out);

// The dispatch order of a laid-out batch's scan_bm section ("bm_place", mrk_batch_submit): slot i of the launch runs item
// disp[i] of the section.  Workgroups are dealt round-robin over the chip's eight XCDs (slot % 8), each with an L2 of its own,
// and a keyword's lines are shared only between workgroups that sit on one XCD and walk the same windows at the same time.
// Owners (the groups, or the queries on the ungrouped layout) are assigned to PLACE_CLASSES classes so that the bytes of the
// distinct keywords per class, summed, are small and the classes' items balanced: owners by items, then bytes, descending,
// each to the class that adds the fewest bytes of keywords new to it under a cap of ceil(total / 8) items + twice the smallest
// owner's (no class under the cap: the lightest), then up to eight sweeps of single moves that lower the sum; ties go to the
// lighter class, then the lower index.  A keyword is a (bitmap, idf) key and costs what group_bm_items charges (windows and
// blocks x 256 B, blocks x 128 B with the nibble plane).  Inside a class the items run by ascending blk_begin, then owner:
// the whole chip walks the corpus as one band of windows.  Slot 8 s + x takes the s-th item of class x; when a class has run
// out, its slots take the next item of the class with the most items left (only there is the affinity lost).
// mode 0: identity; 1: classes + window order; 2: window order alone, dealt as it comes (one class).  Fewer than two owners
// or an empty section: identity, `ran` false.  The slot's XCD is a speed hint: nothing may depend on it.
constexpr uint32_t PLACE_CLASSES = 8;
struct BmPlacement {
  std::vector<uint32_t> disp;        // n_items_kind[0] entries, relative to the section's start
  std::vector<uint8_t> owner_class;  // per owner (group index; ungrouped: owners in the order of their first item, owner_pass names them)
  std::vector<uint32_t> owner_pass;  // ungrouped layout: the owners' pass indexes (grouped: empty)
  uint32_t owner_keys = 0, class_keys = 0; // distinct (owner, keyword) and (class, keyword) pairs; 0 when no placement ran
  uint64_t owner_bytes = 0, class_bytes = 0; // ... and the bytes of those keywords
  bool ran = false;
  bool mismatch = false; // the ranges layout_batch handed out do not add up to the section's items: identity, and an error for the caller
  // scratch of place_bm_items, kept so that a batch's next submit allocates nothing
  struct Own {
    uint32_t items = 0, begin = 0, end = 0, len = 1, nkeys = 0, key[BM_GROUP_TABS] = {};
    uint64_t bytes = 0;
  };
  struct Cur {
    uint32_t next, len, left; // blk_begin of the owner's next piece, its piece length, its pieces left
    uint32_t idx, step, run;  // ... that piece's place in the section, the distance to the one after, and how many pieces that holds for
    uint32_t o, k, tier;
  };
  struct Scratch {
    std::vector<Own> own;
    std::vector<Cur> mem;
    std::vector<std::pair<uint64_t, uint32_t>> keys;
    std::vector<uint64_t> kb;
    std::vector<uint16_t> cnt;
    std::vector<uint32_t> live, slot, by_load, first, rank, counts, fill, own_of, by_own, rest;
  } scratch;
};
void place_bm_items(const DevQuery* head, uint32_t n, const std::vector<DevQuery>& extra, const BatchLayout& lay, bool nibble_plane, int mode,
                    BmPlacement& out);

// A query's decline mask (PackXRowsArgs::declined): bit RowKind k set = the query's exchange row of format k leaves the batch empty
// with MRK_ROW_DECLINED.  status: what plan_query returned for it; sort_bits / order: the batch's SortLoc facts (bits != 0: it is
// sorted or ordered by an attribute; order: 0, or its DevQuery::sort_on when it came as mrk_query.order); orows_wf_run: the submit
// ran with mrk_batch_orows_weight_first on.  A NARROW row is merged by (weight, docid), which answers relevance queries only; a WIDE
// row has no room for a 64-bit key (SORT_ON_ORDER) and no word for the weight in front (SORT_ON_WEIGHT); an ORDER row carries both,
// the latter only where the batch asked for it.  The order bit implies the wide bit, the wide bit the narrow one: some bit is set
// exactly when the narrow bit is.  (A grouped query leaves in none of these three formats -- merging groups adds counts per key,
// which no top-K merge does: its mask is all three bits, set where this function is called -- query_decline_mask.  It travels in
// GROUP rows, whose bit is group_row_decline_bit's, below.)
inline uint32_t row_decline_mask(int status, uint32_t sort_bits, uint32_t order, bool orows_wf_run) {
  const bool off = status != MRK_OK, no_row = order == SORT_ON_ORDER || order == SORT_ON_WEIGHT;
  const bool narrow = off || sort_bits != 0 || no_row, wide = off || no_row, ord = off || (order == SORT_ON_WEIGHT && !orows_wf_run);
  return (narrow ? 1u << ROWS_NARROW : 0u) | (wide ? 1u << ROWS_WIDE : 0u) | (ord ? 1u << ROWS_ORDER : 0u);
}

inline uint32_t query_decline_mask(int status, uint32_t sort_bits, uint32_t order, bool orows_wf_run, bool grouped) {
  return grouped ? (1u << ROWS_NARROW) | (1u << ROWS_WIDE) | (1u << ROWS_ORDER) : row_decline_mask(status, sort_bits, order, orows_wf_run);
}
// The fourth bit of the mask, OR-ed to the three above where a batch fills it: a GROUP row (MRK_GROW_WORDS) carries grouped and
// relevance queries and declines the rest -- a query the planner declined, and a sorted or ordered one.  It implies the narrow bit.
inline uint32_t group_row_decline_bit(int status, uint32_t sort_bits, uint32_t order) {
  return status != MRK_OK || sort_bits != 0 || order != 0 ? 1u << ROWS_GROUP : 0u;
}
// The fifth bit: an AGGREGATE row (MRK_AROW_WORDS) carries what a GROUP row carries and a grouped query's aggregates with it, so a
// query's aggregates do not set it (the batch ORs the GROUP bit for them; this bit it leaves as this function gives it).
inline uint32_t aggr_row_decline_bit(int status, uint32_t sort_bits, uint32_t order) {
  return status != MRK_OK || sort_bits != 0 || order != 0 ? 1u << ROWS_AGGR : 0u;
}

// Least and largest field-weight sum over the masks of the first nwf (<= 32) fields, the empty mask counting as 1
// (ExtRanker_WeightSum_c's "just fake it"): the pruning bins of the weight-sum rankers.
void weight_sum_range(const int32_t* weights, uint32_t nwf, int64_t& rmin, int64_t& rmax);

} // namespace mrk
