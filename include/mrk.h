/*
 * mrk.h -- C-ABI of the MI355X-native match -> rank -> top-K path ("mrk").
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Each entry point names the reference interface it stands in for
 * (paths relative to the Manticore 3.6.1 tree, src/...).
 *
 *   mrk_segment_create   <- what DiskIndexQwordSetup_c binds per index: .spd/.spp/.spe
 *                           readers + skiplist_block_size + the dictionary lookup result
 *                           CSphDictEntry (sphinx.cpp:326-354, 12953-13080; sphinx.h:542-552)
 *   mrk_query (tree)     <- XQNode_t / XQKeyword_t as handed to sphCreateRanker
 *                           (sphinxquery.h:134-286; sphinxsearch.cpp:4167)
 *   mrk_batch_submit     <- sphCreateRanker + the MatchExtended loop
 *                           (sphinxsearch.cpp:4167-4380; sphinx.cpp:12190-12269):
 *                           ExtNode_i::Create, IDF setup, GetMatches() until exhausted
 *   mrk_batch_submit_grouped <- the same with the grouping sorter in place of the plain queue for queries that carry a
 *                           mrk_group: CSphKBufferGroupSorter::PushEx / FinalizeMatches (sphinxsort.cpp:2961-3310)
 *   mrk_result           <- what the caller reads back from ISphMatchSorter:
 *                           Flatten() order + GetTotalCount() (sphinxsort.h:39-133,
 *                           sphinxsort.cpp:627-641, 724) and CSphQueryStats (sphinx.h:2697-2705)
 *   mrk_topk_merge       <- CSphMatchQueue::MoveTo across chunks / shards
 *                           (sphinxsort.cpp:681-710; sphinxrt.cpp:5945-5981)
 *   mrk_idf              <- the IDF block of sphCreateRanker (sphinxsearch.cpp:4317-4361)
 *
 * Threading: a mrk_ctx owns one HIP device, its streams and ONE internal submission thread: every
 * entry point that reaches the HIP runtime posts its work there and sleeps until it has run, so
 * nothing of HIP executes on the caller's stack -- the reference runs rankers on 128 KB coroutine
 * stacks (coroutine.cpp:47) -- and all of a context's host state is touched by one thread only.
 * A mrk_batch is used by one thread at a time; different batches (and segments) of one context
 * may be driven from different threads concurrently.  mrk_batch_wait polls the batch's stream
 * and steps aside for other threads' submits instead of parking the submission thread.
 * MRK_INLINE_HIP=1 in the environment runs everything on the calling thread instead.
 *
 * Errors: every function returns MRK_OK (0) or a negative code; mrk_last_error() gives
 * the message for the calling thread (the reference's convention: no exceptions, error
 * string on the side -- sphinxsearch.cpp:4377-4378).
 */
#ifndef MRK_H
#define MRK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRK_OK 0
#define MRK_E_INVAL (-1)       /* bad argument */
#define MRK_E_UNSUPPORTED (-2) /* query shape / ranker the device path does not cover (yet) */
#define MRK_E_HIP (-3)         /* HIP runtime failure */
#define MRK_E_NOMEM (-4)
#define MRK_E_FORMAT (-5)      /* malformed index bytes */

#define MRK_INVALID_ROWID 0xFFFFFFFFu
#define MRK_MAX_AND_TERMS 8    /* device N-way AND width */
#define MRK_MAX_K 1024         /* device top-K capacity (max_matches default is 1000) */
#define MRK_ALL_FIELDS 0xFFFFFFFFu

/* ESphRankMode order (sphinx.h) */
enum {
  MRK_RANK_PROXIMITY_BM25 = 0,
  MRK_RANK_BM25 = 1,
  MRK_RANK_NONE = 2,
  MRK_RANK_WORDCOUNT = 3,
  MRK_RANK_PROXIMITY = 4,
  MRK_RANK_MATCHANY = 5,
  MRK_RANK_FIELDMASK = 6,
  MRK_RANK_SPH04 = 7
};

/* XQOperator_e subset (sphinxquery.h) */
enum { MRK_OP_TERM = 0, MRK_OP_AND = 1, MRK_OP_OR = 2, MRK_OP_MAYBE = 3, MRK_OP_ANDNOT = 4, MRK_OP_PHRASE = 5,
       MRK_OP_PROXIMITY = 6, /* '"a b c"~N': opt = N */
       MRK_OP_BEFORE = 8, /* 'a << b << c' (ExtOrder_c): the children occur in this order inside one field */
       MRK_OP_QUORUM = 7, /* '"a b c"/N': opt = N (ExtQuorum_c; N = 1 / N >= words as the reference rewrites them) */
       MRK_OP_NEAR = 9,   /* 'a NEAR/N b' (ExtNWay_T<FSMmultinear_c>): opt = N; operands: keywords, phrases, nested NEARs; 3+ operands at the query root only */
       MRK_OP_NOTNEAR = 10, /* 'a NOTNEAR/N b' (ExtNotNear_c): opt = N */
       MRK_OP_SENTENCE = 11, /* 'a SENTENCE b' (ExtUnit_c): both sides inside one sentence of an index_sp = 1 index; the node's term_id = the
                                dictionary slot of the boundary keyword MAGIC_WORD_SENTENCE "\3sentence" (< 0: the index holds none: plain AND) */
       MRK_OP_PARAGRAPH = 12 /* 'a PARAGRAPH b': the same over MAGIC_WORD_PARAGRAPH "\3paragraph" */ };

enum { MRK_HITFMT_PLAIN = 0, MRK_HITFMT_INLINE = 1 }; /* ESphHitFormat */

typedef struct mrk_ctx mrk_ctx;
typedef struct mrk_segment mrk_segment;
typedef struct mrk_batch mrk_batch;

/* CSphDictEntry (sphinx.h:542-552): result of the dictionary lookup for one keyword */
typedef struct {
  uint64_t wordid;       /* m_uWordID (informational) */
  uint64_t doclist_off;  /* m_iDoclistOffset into .spd */
  uint64_t doclist_len;  /* m_iDoclistLength, bytes incl. the 0 terminator */
  uint64_t skiplist_off; /* m_iSkiplistOffset into .spe (valid iff docs > skiplist_block_size) */
  uint32_t docs;         /* m_iDocs */
  uint32_t hits;         /* m_iHits */
} mrk_dict_entry;

/* One index segment (plain index / RT disk chunk) in the reference's v62 byte format */
typedef struct {
  const uint8_t* spd; /* doclists  (host memory; copied to HBM) */
  uint64_t spd_len;
  const uint8_t* spp; /* hitlists */
  uint64_t spp_len;
  const uint8_t* spe; /* skiplists */
  uint64_t spe_len;
  const mrk_dict_entry* dict; /* flat term table indexed by term id (stands in for .spi) */
  uint32_t n_terms;
  uint64_t total_docs;          /* m_iTotalDocuments */
  uint32_t skiplist_block_size; /* index setting; 32 (default) or 128 */
  uint32_t hit_format;          /* MRK_HITFMT_* */
  uint32_t n_fields;            /* schema full-text fields (<= 32 on the device path; the packed path covers all 32, with one extra
                                   plane of field masks above 8 fields) */
  uint32_t rowid_base;          /* global docid = rowid_base + rowid for shard merges; rowid_base + total_docs <= 2^32 (global
                                   rowids are 32 bits), or mrk_segment_create / mrk_segment_validate answer MRK_E_INVAL */
} mrk_segment_desc;

/* XQNode_t flattened: nodes[] + children[] (indices into nodes[]) */
typedef struct {
  int32_t op;          /* MRK_OP_* */
  int32_t n_children;
  int32_t first_child; /* offset into children[] */
  int32_t term_id;     /* leaf: dictionary slot; < 0 = keyword not in the dictionary.  SENTENCE / PARAGRAPH node: the boundary keyword's slot */
  int32_t atom_pos;    /* XQKeyword_t::m_iAtomPos */
  uint32_t field_mask; /* XQLimitSpec_t::m_dFieldMask, low dword */
  float boost;         /* XQKeyword_t::m_fBoost */
  int32_t opt;         /* XQNode_t::m_iOpArg */
  int32_t not_weighted;
  int32_t term_pos;      /* leaf: MRK_TERMPOS_* position modifier (ExtTermPos_T, searchnode.cpp:2259-2405) */
  int32_t field_max_pos; /* leaf: XQLimitSpec_t::m_iFieldMaxPos for MRK_TERMPOS_LIMIT ('@field[N] word') */
} mrk_node;

/* TermPosFilter_e as ExtNode_i::Create derives it (searchnode.cpp:875-878, 1145-1146): '^word' = START, 'word$' = END,
   both = STARTEND, a field position limit = LIMIT (and wins over the anchors) */
enum { MRK_TERMPOS_NONE = 0, MRK_TERMPOS_START = 1, MRK_TERMPOS_END = 2, MRK_TERMPOS_STARTEND = 3, MRK_TERMPOS_LIMIT = 4 };

/* One attribute filter (CSphFilterSettings, sphinx.h:2461-2496) over an integer attribute of the row-wise .spa storage,
   already resolved to the attribute's locator.  All filters of a query must pass (Filter_And); rejected rows never reach
   the ranker or the sorter and are not counted (ExtRanker_c::GetMatches -> CSphIndex_VLN::EarlyReject,
   sphinxsearch.cpp:1055-1064, sphinx.cpp:11903-11917). */
enum { MRK_FILTER_VALUES = 0, MRK_FILTER_RANGE = 1, MRK_FILTER_FLOATRANGE = 2 }; /* SPH_FILTER_VALUES, SPH_FILTER_RANGE, SPH_FILTER_FLOATRANGE */
#define MRK_MAX_FILTERS 2
#define MRK_MAX_FILTER_VALUES 8
typedef struct {
  int32_t kind;                 /* MRK_FILTER_* */
  int32_t bit_offset, bit_count; /* CSphAttrLocator::m_iBitOffset / m_iBitCount (1..32 inside one dword, or 64 dword-aligned) */
  int32_t exclude;              /* m_bExclude: the row passes iff the test fails */
  int32_t has_equal_min, has_equal_max, open_left, open_right; /* RANGE: m_bHasEqualMin/Max, m_bOpenLeft/Right */
  int64_t min_value, max_value; /* RANGE (SphAttr_t is signed 64-bit) */
  const int64_t* values;        /* VALUES: ascending (IFilter_Values::SetValues), <= MRK_MAX_FILTER_VALUES on the device */
  int32_t n_values;
  /* FLOATRANGE over a 32-bit float attribute (Filter_FloatRange, sphinxfilter.cpp:275-300): the row's dword read as a float
     (sphDW2F) against [fmin, fmax] with m_bHasEqualMin / Max; the reference's float filter has no open-sided form */
  float fmin, fmax;
  /* A multi-value attribute (SPH_ATTR_UINT32SET / INT64SET): mva_bits = 32 / 64 (0 = a plain row attribute).  Its values live,
     sorted, in the blob pool (mrk_segment_set_blobs) as blob attribute blob_attr_id of the row's n_blob_attrs
     (CSphAttrLocator::m_iBlobAttrId / m_nBlobAttrs; the row's blob offset is its second attribute, sphGetBlobRowOffset).
     VALUES: any of the doc's values is in the set (Filter_MVAValues_Any_c) or, mva_all, every one is (.._All_c);
     RANGE: some value inside [min, max] (MvaEval_RangeAny) or all of them (MvaEval_RangeAll); sphinxfilter.h:160-240,
     sphinxfilter.cpp:340-383.  A doc without values fails both forms. */
  int32_t mva_bits, mva_all, blob_attr_id, n_blob_attrs;
} mrk_filter;

/* The sorter's order (ISphMatchSorter's comparator, sphinxsort.cpp): relevance = MatchRelevanceLt_fn (weight desc, rowid asc), the
   default; MRK_SORT_ATTR = ONE row attribute of at most 32 bits first -- SPH_SORT_ATTR_DESC / _ASC (MatchAttrLt_fn / MatchAttrGt_fn,
   sphinxsort.cpp:4552-4610: then_weight = 1) and SPH_SORT_EXTENDED of the shapes 'attr' and 'attr, weight()' (MatchGeneric1_fn / 2_fn,
   :4708-4730) --, optionally the weight next, rowid ascending last.  An integer key compares as SphAttr_t does for a zero-extended
   attribute (unsigned), a float key as the dword read as a float (-0.0 == +0.0 falls through to the next key part).
   Declined per query with MRK_E_UNSUPPORTED: a blob-stored attribute (bit_offset < 0), a 64-bit one (bit_count 64, dword-aligned, inside
   the rows the segment holds -- any other 64 is MRK_E_INVAL), a segment without
   attribute rows, a float column that holds a NaN (no strict weak order), cutoff next to a sort, the VLB-direct path.  Locators outside
   the row, bit_count 0 or 33..63, unknown kinds / tie rules: MRK_E_INVAL.  Sorted queries run on the packed block-scan path only. */
enum { MRK_SORT_RELEVANCE = 0, MRK_SORT_ATTR = 1 };
enum { MRK_SORTKEY_INT = 0, MRK_SORTKEY_FLOAT = 1, MRK_SORTKEY_INT64 = 2 /* mrk_order only: signed, as SphAttr_t compares */ };
typedef struct {
  int32_t kind;                  /* MRK_SORTKEY_* */
  int32_t bit_offset, bit_count; /* CSphAttrLocator of a row attribute: 1..32 bits inside one dword */
  int32_t desc;                  /* 1 = descending */
  int32_t then_weight;           /* 0 = attribute, rowid asc;  1 = attribute, weight DESC, rowid asc;  2 = attribute, weight ASC, rowid asc */
} mrk_sort;

/* The wider form of the sorter's order (SPH_SORT_EXTENDED; MatchGeneric1_fn .. 3_fn, sphinxsort.cpp:4708-4753): up to
   MRK_MAX_ORDER_PARTS row attributes, each with its own direction, then the weight as then_weight says (mrk_sort's meaning), rowid
   ascending last.  Accepted shapes:
     - ONE part of kind INT64: bit_count 64, dword-aligned, inside the row; compared as a SIGNED 64-bit integer (SPH_KEYPART_INT
       over a 64-bit locator -- 'ORDER BY id', any bigint column);
     - ONE or TWO parts of kind INT (1..32 bits inside one dword, unsigned) / FLOAT (32 bits).
   One part of <= 32 bits answers exactly as the same spec through mrk_query.sort does.  mrk_query.sort and mrk_query.order both set,
   n_parts outside 1..MRK_MAX_ORDER_PARTS, unknown kinds / tie rules, locators outside the row or straddling a dword, 64 bits that are
   not dword-aligned, INT64 as one of two parts: MRK_E_INVAL, before a row is read.  Declined per query with MRK_E_UNSUPPORTED: a
   blob-stored part (bit_offset < 0), a float part whose column holds a NaN, a segment without attribute rows, cutoff next to an
   order, the VLB-direct path.  A key of more than 32 bits (INT64, two parts) fits no exchange row: such a query leaves in narrow
   AND wide rows with MRK_ROW_DECLINED and no keys.
   The weight in FRONT of the parts (SPH_KEYPART_WEIGHT as key part 0 of MatchGeneric2_fn / 3_fn: 'ORDER BY weight() DESC, attr'):
   then_weight = MRK_ORDER_WEIGHT_FIRST_DESC / _ASC -- the weight, then the parts in their order and directions, rowid ascending last.
   mrk_order keeps its size and layout (callers built against it stay valid): then_weight says where the weight stands, behind the
   parts (0 / 1 / 2) or in front of them, so "in front and behind" cannot be said.  The same shapes of parts; _ASC also takes
   n_parts 0 ('ORDER BY weight() ASC': it reads no attribute row and needs none); _DESC without parts is relevance (leave order NULL)
   and MRK_E_INVAL, like every other value of then_weight.  A weight-first query leaves in narrow and wide rows with
   MRK_ROW_DECLINED, no keys and spec word 0, and so it does in order rows unless the batch was told to carry it there
   (mrk_batch_orows_weight_first, below: bit 3 of the order spec word).  mrk_result.order_key holds the raw parts as for every order
   (NULL without parts). */
#define MRK_MAX_ORDER_PARTS 2
typedef struct {
  int32_t kind;                  /* MRK_SORTKEY_* */
  int32_t bit_offset, bit_count; /* CSphAttrLocator of a row attribute */
  int32_t desc;                  /* 1 = descending */
} mrk_order_part;
typedef struct {
  int32_t n_parts;
  mrk_order_part parts[MRK_MAX_ORDER_PARTS];
  int32_t then_weight;           /* as mrk_sort::then_weight, behind the last part; or MRK_ORDER_WEIGHT_FIRST_*: in front of the first */
} mrk_order;
#define MRK_ORDER_WEIGHT_FIRST 0x100 /* then_weight = this | 1 (weight DESC) or | 2 (weight ASC): the weight leads the order */
#define MRK_ORDER_WEIGHT_FIRST_DESC ( MRK_ORDER_WEIGHT_FIRST | 1 )
#define MRK_ORDER_WEIGHT_FIRST_ASC ( MRK_ORDER_WEIGHT_FIRST | 2 )

/* GROUP BY one integer row attribute (CSphQuery::m_sGroupBy with m_eGroupFunc = SPH_GROUPBY_ATTR; the grouping sorter
   CSphKBufferGroupSorter, sphinxsort.cpp:2961-3310).  The group key is the locator's raw bits (1..32 bits inside one dword: uint,
   timestamp, bool, bit-field), compared unsigned.  Per group the sorter keeps ONE head match and a counter (PushEx, :3148-3205;
   PushIntoExistingGroup, :3112-3145): the head is the group's best match in the default within-group order -- m_sSortBy
   "@weight desc" (searchdsql.cpp:25) / SPH_SORT_RELEVANCE: weight DESC, then global rowid ASC (MatchRelevanceLt_fn) --, @count the
   number of the group's matches that reached the sorter (past dead rows, attribute filters and weight filters; the weight carries
   index_weight).  The groups leave in the order sort_by names -- the group key (@groupby), @count or the head's weight, descending
   or ascending -- then the head's global rowid ascending (MatchGeneric1_fn, :4708-4720; FinalizeMatches, :3233-3300): the best
   min(groups, max_matches) of them, total_found = the number of groups (++m_iTotal on a new group only).
   Exact or declined.  The reference keeps max_matches * GROUPBY_FACTOR (= 4, :2767) groups and then starts to cut the worst
   (CutWorst, :3176), after which its answer depends on the order the matches arrived in.  A query with at most 4 * max_matches
   distinct group values is answered exactly as the reference answers it in any arrival order; one with more is declined WHILE IT
   RUNS: status MRK_E_UNSUPPORTED, a message that names the limit, exchange rows with MRK_ROW_DECLINED -- never a truncated answer.
   Declined at plan time with MRK_E_UNSUPPORTED: a group next to mrk_query.sort / mrk_query.order, cutoff next to a group, a
   blob-stored attribute (bit_offset < 0), a 64-bit one, a segment without attribute rows, the VLB-direct path.  MRK_E_INVAL before a
   row is read: locators outside the row or straddling a dword, bit_count 0 or > 32 (other than an aligned 64 inside the row),
   an unknown sort_by, desc outside 0 / 1.  A grouped query is routed as a sorted one (packed block-scan path; hit-ranked shapes
   through the match queue) and whatever declines a sort declines a group.  Groups of different segments are merged on the device
   through GROUP rows (MRK_GROW_WORDS, below: that merge adds counts per key, which no top-K merge does): a grouped query leaves
   in narrow, wide and order rows with MRK_ROW_DECLINED, no keys and spec word 0.  mrk_batcher_search takes no group. */
enum { MRK_GROUPSORT_KEY = 0, MRK_GROUPSORT_COUNT = 1, MRK_GROUPSORT_WEIGHT = 2 };
typedef struct {
  int32_t bit_offset, bit_count; /* CSphAttrLocator of the group-by attribute */
  int32_t sort_by;               /* MRK_GROUPSORT_*: what orders the groups */
  int32_t desc;                  /* 1 = descending */
} mrk_group;

/* GROUP BY a multi-value attribute (a 32-bit MVA, SPH_ATTR_UINT32SET, in the blob pool): one group per VALUE -- the facet over tags,
   SELECT ..., COUNT(*) FROM idx WHERE MATCH('...') GROUP BY tags.  The reference: MVAGroupSorter_T::Push (sphinxsort.cpp:4113-4156)
   calls PushEx(match, value) for every value of the match's MVA, into the same CSphKBufferGroupSorter a row attribute's groups go to.
   mrk_batch_submit_mva names the attribute as an MVA filter does (mrk_filter: mva_bits, blob_attr_id, n_blob_attrs) next to the
   query's mrk_group, whose sort_by / desc hold and whose bit_offset / bit_count are ignored.
   Pushes: a match that reaches the sorter (past dead rows, attribute filters and weight filters; the weight carries index_weight) is
     pushed once per STORED value of its MVA, into that value's group.  The stored values are neither de-duplicated nor re-sorted: a
     value stored twice counts twice, as the reference's loop does.  A doc without values joins no group.  An MVA filter on the same
     attribute decides whether the doc reaches the sorter, not which of its values form groups: all of them do.
   Per group: the head is the best match by weight DESC, then global rowid ASC; @count is the number of pushes.
   Result: total_found = the number of groups; the best min(groups, max_matches) of them in the order sort_by / desc name.
     mrk_result is unchanged: group_key the value, group_count @count, rowid / weight the head's.
   Limit: more than 4 * max_matches distinct values -- counted over all docs, also when one doc alone carries them -- is declined
     while the query runs, exactly as for a row attribute (MRK_E_UNSUPPORTED, the message names the limit, MRK_ROW_DECLINED).
   Ties: the ONE place where the reference's answer is open.  Groups of a row attribute have distinct heads, so (order part, head
     rowid) is a total order.  One doc may head several groups of an MVA; ordered by @count or by the head's weight, two such groups
     compare equal in MatchGeneric1_fn, and the reference leaves their order -- and which of them falls off at max_matches -- to its
     unstable sort and to the order the matches arrived in.  The device's rule: AMONG GROUPS WHOSE ORDER KEY IS EQUAL THE SMALLER GROUP
     VALUE COMES FIRST, whatever desc says; the same rule decides which group falls off at max_matches, and the merges of group rows
     apply it too, so sharded == unsharded holds under ties.  (Declining ties would decline the ordinary facet: two rare tags on one
     doc tie at count 1.)
   MRK_E_INVAL before a row is read: mva_bits other than 32 / 64, blob_attr_id / n_blob_attrs out of range or not the segment's, rows
   without a blob locator, an mrk_group_mva without an mrk_group, and the group's unknown sort_by / desc.  MRK_E_UNSUPPORTED per query:
   mva_bits == 64 (the group key has 32 bits), a segment without a blob pool (never set, or dropped by a later mrk_segment_set_attrs),
   aggregates next to it (the accumulators would need a slot per pushed value), and everything that declines a group.  GROUP N BY and
   JSON arrays are out of scope.
   Exchange rows: the query leaves in GROUP rows under the spec word of a 32-bit key and is merged as every grouped query is -- counts
   add per value, the better head wins; the other four row kinds decline it. */
typedef struct {
  int32_t mva_bits;     /* 32 (64: declined) */
  int32_t blob_attr_id; /* which of the row's blob attributes */
  int32_t n_blob_attrs; /* how many the row has: the segment's mrk_segment_set_blobs */
} mrk_group_mva;

/* Aggregates of a grouped query: SUM / MIN / MAX of one integer row attribute over the group's matches that reached the sorter --
   the set @count counts.  The reference's grouping sorter carries a list of aggregate functions next to the counter (m_dAggregates,
   sphinxsort.cpp:2608-2693) and updates them on every push (AggrSum_t / AggrMin_t / AggrMax_t, :1902-1979).  Typing, as the
   reference types the select item:
     kind MRK_SORTKEY_INT (1..32 bits inside one dword)  the locator's raw bits, unsigned.  SUM(attr) is SPH_ATTR_INTEGER and runs
         AggrSum_t<DWORD> (:2623): the sum WRAPS modulo 2^32.  MIN / MAX compare unsigned (AggrMin_t<DWORD> :2663, AggrMax_t<DWORD> :2674).
     ... with MRK_AGGR_WIDEN                              the value zero-extended and aggregated as a 64-bit integer: SUM(BIGINT(attr)),
         which people write to avoid the wrap.
     kind MRK_SORTKEY_INT64 (an aligned 64 inside the row, as mrk_order takes it)  signed: AggrSum_t<int64_t> (:2624, the sum in two's
         complement), AggrMin_t<int64_t> (:2664), AggrMax_t<int64_t> (:2675).
   None of these depends on the order the matches arrive in, so an aggregate is exact wherever the group is (the 4 * max_matches limit
   and its run-time decline are the group's).
   Not offered: AVG -- the reference forces it to float and accumulates float in arrival order (sphinxsort.cpp:5980-5984,
   AggrAvg_t<float> :1919-1949): no order-independent answer to be exact against; a caller derives an average from a widened SUM
   and @count.  MRK_SORTKEY_FLOAT sources are declined per query with MRK_E_UNSUPPORTED: a float SUM depends on the arrival order,
   float MIN / MAX depend on it at NaN and +-0.  GROUP_CONCAT, COUNT(DISTINCT) and aggregates over expressions are out of scope.
   order_by: -1 = mrk_group.sort_by orders the groups; 0..n-1 = that aggregate does (ORDER BY SUM(x) DESC), mrk_group.sort_by must
   then be MRK_GROUPSORT_KEY: compared unsigned in the direction mrk_group.desc gives, then by the head's global rowid ascending,
   exactly as @count is.  Only an aggregate with a 32-bit result (an INT source without WIDEN) may order; a 64-bit one is declined
   with MRK_E_UNSUPPORTED (the selection sorts 64-bit keys, half of which is the head's rowid).
   MRK_E_INVAL before a row is read: n outside 1..MRK_MAX_AGGRS, an unknown func, kind or flag, a locator outside the row or
   straddling a dword, a 64 that is not aligned, WIDEN on an INT64 source, order_by out of range or next to another sort_by,
   aggregates without a group.  MRK_E_UNSUPPORTED per query: a FLOAT source, a blob-stored source (bit_offset < 0), a 64-bit order,
   and everything that declines the group.
   Exchange rows: aggregates travel in aggregate rows (MRK_AROW_WORDS, below); the other four kinds decline them -- a query with
   aggregates leaves in GROUP rows, as in narrow, wide and order rows, with MRK_ROW_DECLINED, no entries and spec word 0: the
   group row has no room for the accumulators. */
enum { MRK_AGGR_SUM = 1, MRK_AGGR_MIN = 2, MRK_AGGR_MAX = 3 };
#define MRK_AGGR_WIDEN 1 /* mrk_aggr.flags: an INT source aggregated as a 64-bit integer */
#define MRK_MAX_AGGRS 4
typedef struct {
  int32_t func;                  /* MRK_AGGR_* */
  int32_t kind;                  /* MRK_SORTKEY_INT or MRK_SORTKEY_INT64 */
  int32_t bit_offset, bit_count; /* CSphAttrLocator of the source attribute */
  int32_t flags;                 /* MRK_AGGR_WIDEN or 0 */
} mrk_aggr;
typedef struct {
  int32_t n;        /* 1..MRK_MAX_AGGRS */
  int32_t order_by; /* -1, or the aggregate that orders the groups */
  mrk_aggr a[MRK_MAX_AGGRS];
} mrk_aggrs;

/* CSphQuery fields that reach the ranker + the query tree */
typedef struct {
  const mrk_node* nodes;
  int32_t n_nodes;
  const int32_t* children;
  int32_t root;
  int32_t ranker;               /* MRK_RANK_* (CSphQuery::m_eRanker) */
  int32_t max_matches;          /* K (CSphQuery::m_iMaxMatches) */
  const int32_t* field_weights; /* CSphQueryContext::m_dWeights, NULL => 1 per field */
  int32_t n_weights;
  int32_t index_weight;         /* MatchExtended iIndexWeight, 0 => 1 */
  int32_t plain_idf;            /* CSphQuery::m_bPlainIDF */
  int32_t normalized_tfidf;     /* CSphQuery::m_bNormalizedTFIDF */
  int64_t total_docs_override;  /* CSphQueryContext::m_iTotalDocs (local_df), <= 0: segment's */
  const int64_t* local_docs;    /* per node: m_pLocalDocs override of term docs, < 0 none; or NULL */
  int32_t cutoff;               /* CSphQuery::m_iCutoff (0 = none): the first `cutoff` matches in rowid order are the result set.
                                   <= MRK_MAX_K, packed path, not next to a weight filter; costs a probe launch inside mrk_batch_submit.
                                   Per segment, as MatchExtended counts per disk index; an RT index counts ON across its RAM segments
                                   (PerformFullTextSearch, sphinxrt.cpp:6302-6380): the caller lowers the cutoff by each segment's total_found */
  const mrk_filter* filters;    /* CSphQuery::m_dFilters resolved against the schema; needs mrk_segment_set_attrs */
  int32_t n_filters;            /* <= MRK_MAX_FILTERS on the device */
  /* CSphQueryContext::m_pWeightFilter: filters on the match weight ('WHERE weight() >= N'; Filter_WeightValues /
     Filter_WeightRange, sphinxfilter.cpp:304-320), applied after index_weight and before the sorter (MatchExtended,
     sphinx.cpp:12220-12227); matches they drop are not counted.  kind VALUES / RANGE, exclude, has_equal_min / max;
     the locator fields are ignored.  All must pass. */
  const mrk_filter* weight_filters;
  int32_t n_weight_filters;     /* <= MRK_MAX_FILTERS on the device */
  const mrk_sort* sort;         /* NULL = (weight desc, rowid asc) */
  const mrk_order* order;       /* NULL = as mrk_query.sort says; not next to a sort */
} mrk_query;

typedef struct {
  int32_t n;              /* matches returned, best first (<= max_matches) */
  int64_t total_found;    /* ISphMatchSorter::GetTotalCount() */
  const uint32_t* rowid;  /* n entries, valid until the batch is resubmitted/destroyed */
  const int32_t* weight;
  int32_t status;         /* MRK_OK or MRK_E_UNSUPPORTED for this query */
  const uint32_t* sort_key; /* a query with mrk_query.sort: the primary attribute's raw value (the locator's bits) per returned row; NULL
                               for relevance queries and for mrk_batcher_search (whose rows land in the caller's buffers).  Read from the
                               segment's rows when the result is fetched: no mrk_segment_set_attrs between mrk_batch_submit and mrk_batch_result.  weight is the
                               true weight of every row, also where the weight is no part of the order */
  const uint64_t* order_key; /* a query with mrk_query.order: per returned row the raw 64-bit value of an INT64 part; else the first part's raw
                                value in the high dword and the second's (or 0) in the low dword.  Read from the segment's rows like sort_key,
                                which stays NULL for such a query; NULL for every other query and for mrk_batcher_search */
  const uint32_t* group_key;   /* a grouped query (mrk_batch_submit_grouped): the raw group value of every returned row, whose rowid / weight
                                  are the group's head's; NULL for every other query */
  const uint32_t* group_count; /* ... and @count, the group's matches; NULL likewise */
} mrk_result;

typedef struct {
  float scan_ms;          /* decode+intersect+score kernel, HIP-event time on the batch stream */
  float merge_ms;         /* top-K merge kernel */
  uint64_t algo_bytes;    /* sum over queries of doclist bytes of their terms (reference format) */
  uint64_t n_items;       /* work items (workgroups) launched by the scan kernel */
  uint64_t dev_bytes;     /* the same sum over the format the kernel actually read (packed or .spd) */
  uint32_t packed;        /* 1 = packed-doclist path, 0 = VLB-direct path */
  uint64_t n_cands;       /* packed path: candidates that survived in-scan pruning (all queries) */
  uint64_t n_items_bm;    /* of n_items: every work item that is not a block-scan item -- the two-bitmap AND kernel's, the tree kernel's over
                             bitmap words (n_items_bt) and the generic evaluator's */
  float plan_ms;          /* host: query planning inside mrk_batch_submit */
  float submit_ms;        /* host: whole mrk_batch_submit call */
  uint32_t n_rerun;       /* queries the last mrk_batch_wait ran again alone (their match queue or candidate list was full) */
  uint32_t n_bm_groups[4]; /* "bm_group": groups of 1, 2, 3 and 4 two-bitmap AND queries the last submit ran in one workgroup each */
  uint32_t pk_lean;       /* "pair_scan": 1 = the last submit's block-scan work items ran on the lean one-/two-keyword instance, 0 = on the generic
                             one (or the submit had no such items) */
  uint32_t bm_owner_keys; /* "bm_place": distinct (owner, keyword) pairs of the last submit's two-bitmap AND launch -- an owner is a group, or a
                             query where none were formed -- and ... */
  uint32_t bm_class_keys; /* ... distinct (class, keyword) pairs once the owners were assigned to the eight dispatch classes (bm_place = 2:
                             one class).  Both 0 when no placement ran (bm_place = 0, fewer than two owners, no such launch) */
  uint32_t n_items_bt;    /* "bt_cover_inv" / "bt_phrase": of n_items_bm, the work items of the tree kernel over bitmap words (boolean trees and
                             the candidates of root phrases of common words); 0 on the VLB-direct path */
  uint32_t mq_chunks[3];  /* match-queue chunks the planner sized in the last submit for queue 0 (the lean rank pass: plain boolean trees under a
                             hit ranker), 1 (the full hit pass: PHRASE / PROXIMITY / BEFORE / NEAR / NOTNEAR nodes, position modifiers) and 2 (the
                             generic evaluator); 0 = that rank launch did not run.  All three are 0 on the VLB-direct path */
  uint64_t bm_words_queued; /* "bm_wmax": non-empty match words the two-bitmap AND kernel queued for unpacking and scoring in the last submit, ... */
  uint64_t bm_words_pruned; /* ... and those it dropped because the best weight the word's tf classes allow lies behind the query's pruning
                               threshold.  Counted for the queries the bound applies to (BM25, relevance order, no field limits, a segment with
                               the plane); both 0 otherwise.  Reruns of overflowed queries are not counted */
} mrk_batch_stats;

const char* mrk_last_error(void);

int mrk_ctx_create(int device, mrk_ctx** out);
/* Destroy a context's segments, batches and batchers BEFORE the context: their destructors run on its submission thread.
   The context counts them: with any still alive the call destroys nothing and returns MRK_E_INVAL (the message says how many);
   destroy them and call again.  (Until round 3 this was a comment only: a segment or batch destroyed after its context posted
   its destructor to a thread that no longer existed and waited forever.) */
int mrk_ctx_destroy(mrk_ctx* ctx);
/* tunables: "item_bytes" (work-item size target); "pack" (1 = build packed doclists at segment
   load, default); "path" (0 = packed when present, 1 = VLB-direct, 2 = packed only);
   "bitmap_inv" (keywords found in >= 1/bitmap_inv of a segment's docs also get a doc-set bitmap,
   used by the two-bitmap AND kernel; default 64, 0 = off; read at segment load and at submit);
   "attr_seq" (1 = keywords with a bitmap also get their tf / field bytes as two bytes per posting in slot order, which the two-bitmap
   AND kernel gathers from instead of the block decoder's interleaved words: the docs of a 128-byte line are then scored together and
   the line is fetched once, -2.7 % on the headline launch; +2 bytes per posting up to the last such keyword; default 1; read at
   segment load);
   "bm_wmax" (1 = keywords with a bitmap also get one nibble per 32-rowid bitmap word, the largest hit count among the keyword's postings in
   that word capped at 15; the two-bitmap AND kernel computes from the two nibbles of a match word the best weight any match in it can
   have and neither unpacks the word nor fetches its tf / field bytes when that weight lies behind the query's pruning threshold --
   exact results, BM25 in relevance order without field limits and with a positive index_weight; + 1/8 of the bitmaps' bytes, and every
   bitmap then starts at a multiple of four windows (up to 768 B of padding per keyword); 0 = no plane, bitmaps and kernel as before;
   default 1; read at segment load; mrk_batch_stats.bm_words_queued / bm_words_pruned count the words);
   "attr_nibbles" (1 = segments with <= 4 fields also get a one-byte tf/field plane for the bitmap kernel's gathers:
   28 % fewer bytes per dense x dense query, +14 % queries/s on the 100 M-doc bench, +1 byte per posting; default 0 --
   see DESIGN.md section 6; read at segment load);
   "bm_target_items" / "bt_target_items" (cap of the work items per launch the window ranges of the two-bitmap AND kernel / of the tree
   kernel over bitmap words are cut into, defaults 2^20 / 6144) and "bm_min_windows" (windows per work item of the AND kernel, default
   256; 128 before "bm_place": since work items of different queries interleave -- "item_order", a mask: 1 block scan, 2 bitmap AND, 4 bitmap trees, 8 also in
   batches that feed the hit pass; default 7 -- small items are the fast ones); "pk_min_items" (a batch with fewer block-scan work items
   has its block ranges cut finer, default 2048; 1 = the planner's items stay as they are);
   "p2_max_blocks" (a launch on the lean block-scan instance -- "pair_scan" -- keeps no work item longer than this many driver blocks,
   a multiple of the 4 waves of a workgroup: a wave there is a chain of dependent round trips per driver block, and the launch lasts as
   long as its longest waves; part of the same recut as "pk_min_items", so off with pk_min_items = 1; 0 = no cap; default 4, one block per
   wave; read at submit; a speed hint only);
   "pair_scan" (1 = a batch whose block-scan launch needs none of the generic kernel's machinery -- queries of one or two keywords under
   NONE / BM25 / single-keyword PROXIMITY, no trees, phrases, position modifiers, filters or sort, a segment of <= 8 fields packed with
   bitmap_inv != 0 -- runs that launch on a lean instance of the kernel: twice the waves per SIMD and a shorter chain of dependent loads per
   wave; 0 = always the generic instance; default 1; read at submit; mrk_batch_stats.pk_lean says which one ran);
   "bm_group" (1 = a batch's two-bitmap AND queries that share a keyword run in one workgroup, a wave per member, so the shared
   keyword's bitmap and tf/field lines are fetched once per CU; 0 = a workgroup per query; default 1; read at submit);
   "bm_place" (the order the work items of that kernel are dispatched in, read at submit; a speed hint only: results do not depend on
   it.  0 = the layout's piece-major order.  2 = by ascending window, then owner -- an owner is a group, or a query where none were
   formed: the whole chip walks the corpus as one band of windows; the default, measured together with bm_min_windows = 256 at +7 to +9 %
   queries/s on the 100 M-doc bench.  1 = workgroups are dealt round-robin over the chip's eight XCDs, each with an L2 of its own: the owners
   are assigned to eight classes so that a class holds few distinct keywords and the classes hold about as many work items, slot 8 s + x
   of the launch runs the s-th work item of class x, and every class runs its items by ascending window.  Measured: it takes a fifth of
   the L2 misses away and the launch is 5 to 35 % SLOWER, because equal item counts are not equal times and each XCD runs its own
   slots -- DESIGN.md section 6; an experiment setting.  mrk_batch_stats.bm_owner_keys / bm_class_keys count the keywords before and after);
   "bm_place_min_items" (launches of that kernel with fewer work items keep the layout's order: the order costs host time per work item and
   a short launch is over before the band forms; default 16384, about a 50 M-doc segment under 256 queries);
   "prox_prune" (1 = proximity rankers: matches whose weight upper bound cannot reach the top K skip the hit pass, default);
   "prox_bound_keywords" (0 = that bound takes a proximity run to be as long as the field's hits allow: always sound, default;
   1 = as long as the number of keywords in the field -- tighter, and sound where hits of different keywords at ONE position reach
   the ranker in query-position order: indexes whose field-end flag belongs to the position, which is what the reference's indexer
   writes (sphinx.cpp:22424-22430), or that carry no field-end flags; the caller's statement about the context's indexes, read at submit);
   "exchange_part" (1 = mrk_shard_exchange partitions the merge by query, default), "exchange_self_rccl" (1 = a one-rank exchange
   still goes through RCCL, default 0);
   "bt_cover_inv" (boolean trees whose candidate cover -- the keywords whose doc lists together hold every possible match --
   names >= 1/bt_cover_inv of the segment's docs are evaluated on doc-set bitmap words, 8192 rowids per step, instead of
   block by block; default 1024 -- a pure AND of keywords only from 1/32 --, 0 = never; read at submit);
   "bt_phrase" (1 = a root PHRASE / PROXIMITY whose rarest word holds >= 1/bt_cover_inv of the docs takes its candidates -- the AND of
   its words -- from the bitmap words too, default; 0 = block walk);
   "mq_max_chunks" (cap of a batch's match queue -- matched docs of hit-ranked queries on their way to the ranking kernel -- in
   chunks of 64 docs / 1792 bytes, default 2^20; queries that outgrow it are rerun one by one by mrk_batch_wait);
   "gen_lane_hits" / "gen_spill_mb" (the generic per-doc evaluator -- query shapes the specialised hit passes do not take: more
   than four keywords under a hit ranker, phrases of five and more words, BEFORE / NEAR / NOTNEAR over phrases, groups and
   quorums, several such nodes -- keeps each node's hit list of the doc at hand in HBM: 16-byte hits per evaluator lane
   (default 256 x 131072 lanes = 512 MB) and a shared area for longer lists (default 1024 MB); allocated with the first
   batch that holds such a query; a query that outgrows them fails with MRK_E_UNSUPPORTED, it is never truncated);
   returns MRK_E_INVAL for unknown keys */
int mrk_ctx_set(mrk_ctx* ctx, const char* key, int64_t value);

int mrk_segment_create(mrk_ctx* ctx, const mrk_segment_desc* desc, mrk_segment** out);
/* The host-only half of mrk_segment_create, no device needed: the descriptor's limits, every skiplist, and a walk of
   every doclist (entries decode, rowids ascend and stay below total_docs, hitlist offsets stay inside .spp, the
   terminator sits where the dictionary's doc count says).  MRK_OK, or the error mrk_segment_create would return --
   it runs the same checks on whatever the load-time transcode did not already walk, so that untrusted bytes never
   become an out-of-bounds device read. */
int mrk_segment_validate(const mrk_segment_desc* desc);
void mrk_segment_destroy(mrk_segment* seg);
/* Dead-row map of the segment (DeadRowMap_c, killlist.h:22-46: bit rowid&31 of DWORD rowid>>5), copied
   to the device; dead rows are dropped right after ranking, before the sorter, and do not count as found
   (CSphIndex_VLN::MatchExtended, sphinx.cpp:12213-12217).  bitmap = NULL clears the map.  The call waits
   for the context's running batches, so a search sees either the old or the new map. */
int mrk_segment_set_dead_rows(mrk_segment* seg, const uint32_t* bitmap, uint64_t n_rows);
/* Row-wise attribute storage (.spa: CSphRowitem rows[n_rows][stride], sphinx.cpp GetDocinfoByRowID) copied to HBM for the
   filters of mrk_query; rows = NULL drops it.  Waits for the context's running batches like mrk_segment_set_dead_rows.
   A blob pool the segment holds (mrk_segment_set_blobs) was walked against the OLD rows' blob offsets: every call here drops it,
   and MVA filters are declined (MRK_E_UNSUPPORTED, "need the segment's blob pool") until mrk_segment_set_blobs is called again. */
int mrk_segment_set_attrs(mrk_segment* seg, const uint32_t* rows, uint32_t stride_dwords, uint64_t n_rows);
/* The blob pool of the attribute storage (.spb file / RtSegment_t::m_dBlobs: per row a blob row = length-size byte, cumulative
   lengths, data; attribute.cpp:495-513) copied to HBM for MVA filters.  Call it AFTER mrk_segment_set_attrs: the blob row of every
   row the segment HOLDS is walked here once (offset, header and lengths inside the pool), so that untrusted bytes never become an
   out-of-bounds device read -- the kernels follow the blob offsets of those rows and of no others.  rows / stride / n_rows = the
   very rows given to mrk_segment_set_attrs: MRK_E_INVAL when the segment holds no rows, or when they differ from the ones it holds
   (stride, or any dword of the segment's rows); MRK_E_FORMAT when a blob row leaves the pool.  Nothing is installed then.
   pool = NULL drops it. */
int mrk_segment_set_blobs(mrk_segment* seg, const uint8_t* pool, uint64_t pool_len, uint32_t n_blob_attrs, const uint32_t* rows,
                          uint32_t stride_dwords, uint64_t n_rows);
/* device bytes held, and the reference-format doclist bytes of one term */
uint64_t mrk_segment_device_bytes(const mrk_segment* seg);

/* ---- the batching front: ONE query per caller, common launches ----------------------------------------------------------
   searchd runs one ranker per (query x index) on a pool of workers (SearchHandler_c::RunLocalSearches, searchd.cpp:5596-5797);
   a ranker that submits a batch of one pays a launch chain per query.  A batcher (one per index / context) lets the workers'
   queries meet: mrk_batcher_search enqueues the caller's query and sleeps (mutex + condition variable: nothing of HIP on the
   caller's stack) until a driver thread has sent it down -- together with everything else that arrived while the device was
   busy with the launch before, up to max_batch queries of the same segment per mrk_batch_submit, three launches in flight --
   and copied its rows into the caller's own buffers (rowid_out / weight_out, cap entries; res->rowid / res->weight point
   there).  max_wait_us: how long an IDLE device waits for a batch to fill up (0 = launch at once; under load arrivals queue
   behind the running launch anyway).  A query the planner refuses with MRK_E_INVAL fails alone: the others of its launch are
   rerun one by one.  Returns MRK_OK with res->status = the query's own status (MRK_E_UNSUPPORTED = keep the CPU ranker). */
typedef struct mrk_batcher mrk_batcher;
typedef struct {
  uint64_t launches;   /* mrk_batch_submit calls */
  uint64_t queries;    /* queries answered */
  uint32_t max_batch;  /* most queries one launch carried */
  double submit_ms;    /* driver thread: time inside mrk_batch_submit, in all */
  double collect_ms;   /* ... inside mrk_batch_wait + handing the rows out */
  double flight_ms;    /* sum over launches of submit-return -> found complete */
} mrk_batcher_stats;
int mrk_batcher_create(mrk_ctx* ctx, uint32_t max_batch, uint32_t max_wait_us, mrk_batcher** out);
void mrk_batcher_destroy(mrk_batcher* b);
int mrk_batcher_search(mrk_batcher* b, mrk_segment* seg, const mrk_query* q, uint32_t* rowid_out, int32_t* weight_out, int32_t cap, mrk_result* res);
int mrk_batcher_stats_get(mrk_batcher* b, mrk_batcher_stats* out);

int mrk_batch_create(mrk_ctx* ctx, uint32_t max_queries, mrk_batch** out);
void mrk_batch_destroy(mrk_batch* b);
/* plan on host, copy descriptors, launch kernels, start the result copy; returns at once */
int mrk_batch_submit(mrk_batch* b, mrk_segment* seg, const mrk_query* queries, uint32_t n_queries);
/* mrk_batch_submit with a group per query (sphCreateQueue picking the grouping sorter for a query with m_sGroupBy,
   sphinxsort.cpp): groups[i] == NULL = query i is not grouped; groups == NULL = mrk_batch_submit */
int mrk_batch_submit_grouped(mrk_batch* b, mrk_segment* seg, const mrk_query* queries, const mrk_group* const* groups, uint32_t n_queries);
/* ... and with aggregates per grouped query (mrk_aggrs, above): aggrs[i] == NULL = query i has none; aggrs == NULL =
   mrk_batch_submit_grouped.  Aggregates without a group are MRK_E_INVAL */
int mrk_batch_submit_aggr(mrk_batch* b, mrk_segment* seg, const mrk_query* queries, const mrk_group* const* groups, const mrk_aggrs* const* aggrs, uint32_t n_queries);
/* ... and with a multi-value group attribute per grouped query (mrk_group_mva, above): mvas[i] == NULL = query i as before; mvas ==
   NULL = mrk_batch_submit_aggr.  mvas[i] without groups[i] is MRK_E_INVAL */
int mrk_batch_submit_mva(mrk_batch* b, mrk_segment* seg, const mrk_query* queries, const mrk_group* const* groups, const mrk_aggrs* const* aggrs,
                         const mrk_group_mva* const* mvas, uint32_t n_queries);
/* The aggregates of query i's returned rows, after mrk_batch_wait: *values = n x *n_aggrs words, row-major, in the order of the result's
   rows (mrk_batch_result); a 32-bit result zero-extended, a 64-bit one the integer's bits.  NULL / 0 for every query without
   aggregates and for a failed one.  Valid until the batch is resubmitted or destroyed */
int mrk_batch_result_aggrs(mrk_batch* b, uint32_t i, const uint64_t** values, int32_t* n_aggrs);
/* block until the results of the last submit are in host memory; a query that fails here (its result's status != MRK_OK,
   e.g. out of generic-evaluator memory) leaves the reason in mrk_last_error() */
int mrk_batch_wait(mrk_batch* b);
/* has the device finished the last submit?  MRK_OK = yes (mrk_batch_wait returns without blocking), 1 = not yet.  A stream
   query on the CALLING thread (no hop to the submission thread: a polling loop must not queue behind other callers'
   submits): call it from an ordinary thread, not from a coroutine stack. */
int mrk_batch_test(mrk_batch* b);
int mrk_batch_result(mrk_batch* b, uint32_t q, mrk_result* out);
int mrk_batch_stats_get(mrk_batch* b, mrk_batch_stats* out);
/* device-resident partial top-K of the last submit, for shard merges without a host hop:
   keys[q*MRK_MAX_K + i] = ((weight ^ 0x80000000) << 32) | ~(rowid_base + rowid), sorted
   descending; counts[q]; totals[q].  Valid after mrk_batch_wait.  The keys of a query with mrk_query.sort stand in the
   sorter's order; the NARROW rows' merges (mrk_topk_merge*, mrk_topk_merge_rows*, mrk_shard_exchange) order by
   (weight, docid) only, so such a query's narrow exchange row leaves with MRK_ROW_DECLINED.  The WIDE rows below
   (MRK_SROW_WORDS, mrk_batch_export_srows, mrk_topk_merge_srows*, mrk_shard_exchange_srows) carry the mapped sort key of every
   entry and answer a sorted query across segments and shards exactly; the ORDER rows further below (MRK_OROW_WORDS) do the
   same for a query ordered by a 64-bit key (mrk_query.order), which narrow and wide rows decline. */
int mrk_batch_device_results(mrk_batch* b, const uint64_t** keys, const uint32_t** counts, const uint64_t** totals);

/* copy those three arrays into caller-owned device buffers (e.g. tensors handed to RCCL);
   any pointer may be NULL; synchronous */
int mrk_batch_export_device(mrk_batch* b, uint64_t* keys_dst, uint32_t* counts_dst, uint64_t* totals_dst);

/* Shard exchange in one buffer: a row of MRK_ROW_WORDS u64 per query = MRK_MAX_K keys (as above, zero
   padded) | count | total_found.  mrk_batch_export_rows writes the last submit's results as rows into a
   caller-owned DEVICE buffer [n_queries][MRK_ROW_WORDS] (e.g. the tensor handed to one RCCL all-gather) and
   returns when the copy is done; mrk_topk_merge_rows merges rows_all[n_lists][n_queries][MRK_ROW_WORDS]
   (device) into out_rows[n_queries][MRK_ROW_WORDS]: best k keys per query, totals added up
   (CSphMatchQueue::MoveTo, sphinxsort.cpp:681-710). */
#define MRK_ROW_WORDS (MRK_MAX_K + 2)
/* flag bits in a row's total_found word; mrk_topk_merge_rows ORs them through (the counts in the low 62 bits add up):
   MRK_ROW_RERUN    a shard's candidate list overflowed and the row left before mrk_batch_wait reran the query: call
                    mrk_batch_wait + mrk_batch_export_rows on that shard's batch and exchange / merge again;
                    Only a candidate-list overflow leaves with this bit: it is the one condition a rerun repairs;
   MRK_ROW_DECLINED a shard declined the query (MRK_E_UNSUPPORTED there): the merged row is not an answer.  That covers the
                    declines found while the query ran (a doc with more live phrase states than the kernels keep, the generic
                    evaluator out of hit-list memory): the kernels write such a row with this bit, no keys and count 0 themselves,
                    so the standing row carries it before mrk_batch_wait and the exported row after it, in all three formats. */
#define MRK_ROW_RERUN (1ull << 63)
#define MRK_ROW_DECLINED (1ull << 62)
int mrk_batch_export_rows(mrk_batch* b, uint64_t* rows_dst);
/* standing order: every later submit also writes its rows to rows_dst (device, [max_queries][MRK_ROW_WORDS]) on the
   batch's own stream right behind the selection kernel -- valid after mrk_batch_wait, no device work at collection
   time.  NULL cancels it. */
int mrk_batch_set_rows_dst(mrk_batch* b, uint64_t* rows_dst);
/* (A query whose candidate list overflowed is rerun by mrk_batch_wait; a row that left through the standing export
   before that carries no keys and MRK_ROW_RERUN: ask that shard again, see above.) */
/* record a caller-owned hipEvent_t on the batch's stream, i.e. behind everything the last submit queued there
   (selection, standing rows export, result copies): lets another stream (RCCL's) wait for the rows without the host */
int mrk_batch_record_event(mrk_batch* b, void* hip_event);
int mrk_topk_merge_rows(mrk_ctx* ctx, const uint64_t* rows_all, uint32_t n_lists, uint32_t n_queries, uint32_t k,
                        uint64_t* out_rows);

/* Stream-ordered form for pipelined shard merges (nothing blocks the host): the merge is queued on the context's
   merge stream behind `wait_event` (a hipEvent_t recorded by the producer of rows_all, e.g. on the RCCL stream;
   NULL = none) and completion is marked in `slot` (0..MRK_MERGE_SLOTS-1); mrk_merge_wait blocks until that slot's
   work is done.  out_rows may be device memory or PINNED HOST memory (hipHostMalloc / a pinned torch tensor): the
   merge kernel then writes the merged rows straight into host memory (multi-MiB device-to-host hipMemcpyAsync calls
   were seen to block the calling thread for 0.1-0.5 ms; a kernel writing over PCIe does not). */
#define MRK_MERGE_SLOTS 8
int mrk_topk_merge_rows_async(mrk_ctx* ctx, const uint64_t* rows_all, uint32_t n_lists, uint32_t n_queries, uint32_t k,
                              uint64_t* out_rows, void* wait_event, uint32_t slot);
int mrk_merge_wait(mrk_ctx* ctx, uint32_t slot);

/* ------------------------------------------------------------------------------------
 * The shard exchange inside the library (one process per GPU, segments = rowid ranges): RCCL over xGMI, loaded at run
 * time; a C / C++ host needs no Python for it.  Stands in for SearchHandler_c::SetupLocalDF (searchd.cpp:5869-5990) and
 * the merge of per-chunk sorters (sphinxsort.cpp:681-710, sphinxrt.cpp:5945-5950) across the local indexes of one node.
 *
 *   rank 0: mrk_comm_unique_id(id), ship the MRK_COMM_ID_BYTES to the other ranks by any means (file, socket, MPI ...);
 *   every rank: mrk_comm_init(ctx, id, n_ranks, rank)            -- collective, like ncclCommInitRank;
 *   once per index:  mrk_comm_allreduce_i64(ctx, docs, n)       -- per-keyword document counts and the document total,
 *                    summed over the shards: the values of mrk_query.local_docs / total_docs_override (local_df);
 *   per batch:       mrk_batch_set_rows_dst(batch, rows) once, then after each mrk_batch_submit
 *                    mrk_shard_exchange(ctx, batch, rows, n_queries, k, out_rows, slot)
 *                    queues event -> all-gather of the rows -> merge kernel -> out_rows (device or pinned host memory)
 *                    as one stream-ordered chain and returns at once; mrk_merge_wait(ctx, slot) blocks until out_rows is
 *                    written.  Rows carry MRK_ROW_RERUN / MRK_ROW_DECLINED through the merge (see above).
 * ---------------------------------------------------------------------------------- */
#define MRK_COMM_ID_BYTES 128
int mrk_comm_unique_id(uint8_t id_out[MRK_COMM_ID_BYTES]);
int mrk_comm_init(mrk_ctx* ctx, const uint8_t id[MRK_COMM_ID_BYTES], int n_ranks, int rank);
void mrk_comm_destroy(mrk_ctx* ctx); /* also done by mrk_ctx_destroy */
int mrk_comm_allreduce_i64(mrk_ctx* ctx, int64_t* values, uint64_t n);
int mrk_shard_exchange(mrk_ctx* ctx, mrk_batch* batch, const uint64_t* rows, uint32_t n_queries, uint32_t k, uint64_t* out_rows,
                       uint32_t slot);
/* The exchange is PARTITIONED BY QUERY (round 3; ctx key "exchange_part", default 1; needs ncclSend / ncclRecv in the loaded
   RCCL, <= 8 ranks -- else the all-gather form, where every rank receives and merges everything): rank r owns the queries
   mrk_shard_slice(n_queries, n_ranks, r) = [first, first + count), per = ceil(n_queries / n_ranks) each.  Every rank sends each
   owner its rows of the owner's queries (one grouped all-to-all of row slices), merges its own slice and writes
   out_rows[first .. first + count) -- the other rows of out_rows are not touched.  Bytes into a GPU and merge work per GPU are
   1 / n_ranks of the all-gather form's.  "Some shard flagged a row" (MRK_ROW_RERUN / MRK_ROW_DECLINED) is no longer visible in
   every rank's rows: two dwords -- any row flagged RERUN / DECLINED, on any rank -- travel through one small all-reduce behind
   the merge; mrk_shard_flags reads them after mrk_merge_wait (every rank sees the same values and takes the same repair path).
   mrk_shard_partitioned: 1 if mrk_shard_exchange on this context partitions. */
int mrk_shard_slice(uint32_t n_queries, int n_ranks, int rank, uint32_t* first, uint32_t* count);
int mrk_shard_flags(mrk_ctx* ctx, uint32_t slot, uint32_t* rerun_any, uint32_t* declined_any);
int mrk_shard_partitioned(mrk_ctx* ctx);
/* what a rank of the partitioned exchange does with its receive buffer, callable on its own (tests; a host with its own
   transport): rows_recv[n_lists][list_stride][MRK_ROW_WORDS] (device), the rank's `count` queries -> out_rows[first + q].
   n_lists <= 8.  Synchronous. */
int mrk_topk_merge_rows_part(mrk_ctx* ctx, const uint64_t* rows_recv, uint32_t n_lists, uint32_t list_stride, uint32_t first, uint32_t count,
                             uint32_t k, uint64_t* out_rows);

/* ------------------------------------------------------------------------------------
 * Wide exchange rows: sorted queries (mrk_query.sort) across segments and shards.  One row of MRK_SROW_WORDS u64 per query:
 *   [0 .. MRK_MAX_K-1]         the keys of the narrow row, in the sorter's order
 *   [MRK_MAX_K] [MRK_MAX_K+1]  count | total_found with MRK_ROW_RERUN / MRK_ROW_DECLINED, as in the narrow row
 *   [MRK_MAX_K+2 ..]           MRK_MAX_K u32 (two per word, entry 2 j in the low half): entry i = the order-preserving mapped
 *                              key of keys[i]'s primary attribute; zero past count
 *   [MRK_SROW_WORDS-1]         the sort spec word: 0 = a relevance query (the u32 plane is zero and ignored); else
 *                              bit 0 sorted | bit 1 float (else unsigned integer) | bit 2 desc | bits 4-5 then_weight |
 *                              bits 8-13 bit_count -- all that decides whether two shards' mapped keys and tie rules compare,
 *                              and nothing of where a segment stores the column
 * The merge orders a sorted query's entries as the unsharded sorter does: mapped key, then the weight as then_weight says (or not
 * at all), then GLOBAL docid (rowid_base + rowid) ascending; a relevance query's (spec 0) exactly as mrk_topk_merge_rows does.
 * Totals add up and the two flag bits are OR-ed through.  Lists of one query whose spec words differ (a sorted row next to a
 * relevance row included), or a sorted query that some list carries with MRK_ROW_DECLINED, give a merged row with
 * MRK_ROW_DECLINED and no keys: never a mis-ordered answer.  At most 8 lists.  Relevance queries travel in wide rows too, so a
 * mixed batch needs one exchange.  Each function is the wide twin of the narrow one above, argument for argument.
 * A batch has ONE standing destination: mrk_batch_set_srows_dst while a narrow one stands (or the reverse) is MRK_E_INVAL; with
 * a narrow standing destination a sorted query still leaves with MRK_ROW_DECLINED.  After an overflow rerun (MRK_ROW_RERUN),
 * mrk_batch_wait + mrk_batch_export_srows hand out the repaired row, mapped keys included.
 * ---------------------------------------------------------------------------------- */
#define MRK_SROW_WORDS (MRK_ROW_WORDS + MRK_MAX_K / 2 + 1)
int mrk_batch_export_srows(mrk_batch* b, uint64_t* srows_dst);
int mrk_batch_set_srows_dst(mrk_batch* b, uint64_t* srows_dst);
int mrk_topk_merge_srows(mrk_ctx* ctx, const uint64_t* srows_all, uint32_t n_lists, uint32_t n_queries, uint32_t k, uint64_t* out_srows);
int mrk_topk_merge_srows_async(mrk_ctx* ctx, const uint64_t* srows_all, uint32_t n_lists, uint32_t n_queries, uint32_t k,
                               uint64_t* out_srows, void* wait_event, uint32_t slot);
int mrk_topk_merge_srows_part(mrk_ctx* ctx, const uint64_t* srows_recv, uint32_t n_lists, uint32_t list_stride, uint32_t first, uint32_t count,
                              uint32_t k, uint64_t* out_srows);
int mrk_shard_exchange_srows(mrk_ctx* ctx, mrk_batch* batch, const uint64_t* srows, uint32_t n_queries, uint32_t k, uint64_t* out_srows,
                             uint32_t slot);
/* host only: the raw attribute value (the locator's bits; a float's bit pattern) behind a mapped key of a row with this spec
   word.  The map folds a float's -0.0 onto +0.0, so -0.0 reads +0.0. */
uint32_t mrk_sort_unmap_key(uint64_t spec_word, uint32_t mapped);

/* ------------------------------------------------------------------------------------
 * Order rows: queries ordered by a 64-bit key (mrk_query.order: one INT64 attribute, or two attributes of <= 32 bits) across
 * segments and shards.  Narrow and wide rows decline such a query (its mapped key has 64 bits); an order row carries it.  One row
 * of MRK_OROW_WORDS u64 per query:
 *   [0 .. MRK_MAX_K-1]         the keys of the narrow row, in the sorter's order
 *   [MRK_MAX_K] [MRK_MAX_K+1]  count | total_found with MRK_ROW_RERUN / MRK_ROW_DECLINED, as in the narrow row
 *   [MRK_MAX_K+2 ..]           MRK_MAX_K u64: entry i = the 64-bit order-preserving mapped key of keys[i] (larger = better:
 *                              map32(first part) << 32 | map32(second part)); zero past count
 *   [MRK_OROW_WORDS-1]         the order spec word: 0 = a relevance query (the plane is zero and ignored); else
 *                              bit 0 ordered | bit 1 wide (a 64-bit key) | bit 2 INT64 | bit 3 weight-first | bits 4-5 then_weight |
 *                              part p in the 16 bits from bit 8 + 16 p: bit 0 float | bit 1 desc | bit 2 signed (the high dword
 *                              of an INT64) | bits 4-9 bit_count -- all that decides whether two shards' mapped keys and tie
 *                              rules compare and how a mapped key turns back into a raw value, nothing of where a segment
 *                              stores the columns
 * A mrk_query.sort query travels in order rows too, and so does a one-part order of <= 32 bits (which is that sort): its 32-bit
 * mapped key stands in the high dword over a zero low dword and its spec has the wide bit clear.  Relevance queries travel with
 * spec 0 and a zero plane, so a mixed batch needs one exchange.  The merge orders an ordered query's entries as the unsharded
 * sorter does: mapped key, then the weight as then_weight says (or not at all), then GLOBAL docid ascending; a relevance query's
 * exactly as mrk_topk_merge_rows does (words 0 .. MRK_MAX_K+1 of its merged row equal that merge's).  Totals add up and the two
 * flag bits are OR-ed through.  A shard whose planner declined the query (e.g. a NaN in that shard's float part) sends it with
 * MRK_ROW_DECLINED, no keys and spec word 0; such a list's spec word is not compared.  The lists that answer the query must agree
 * in every bit of their spec words.  If they do not, or if the query is ordered and some list carries it with MRK_ROW_DECLINED,
 * the merged row has MRK_ROW_DECLINED, no keys and the answering lists' spec word (that of the first one, if they differ; the same
 * row whichever list declined): never a mis-ordered answer.  At most 8 lists.  Each function is the twin of the wide one above, argument for argument.  A batch has ONE
 * standing destination of the three kinds: setting a second kind while one stands is MRK_E_INVAL.  After an overflow rerun
 * (MRK_ROW_RERUN), mrk_batch_wait + mrk_batch_export_orows hand out the repaired row, mapped keys included.
 * Weight-first orders (MRK_ORDER_WEIGHT_FIRST_*).  Bit 3 of the spec word says that the weight leads the order; bits 4-5 then hold
 * the WEIGHT's direction, 1 DESC / 2 ASC (0 and 3 are no valid spec), and every other field reads as without the bit: one part of
 * <= 32 bits (wide clear, its key in the high dword), two parts (wide), one INT64 (wide | INT64), or no part at all ('weight() ASC'
 * alone: both part fields zero, the plane all zero).  The plane holds the parts' 64-bit mapped key; the merge orders such a query's
 * entries by the weight as the direction says, then the mapped key, then GLOBAL docid ascending.  A spec with bit 3 and direction
 * 0 or 3 merges to MRK_ROW_DECLINED, no keys and that spec word; a weight-first list next to any other spec is a mismatch as above.
 * A merger that predates bit 3 cannot read such rows, so a batch writes them only when told to: mrk_batch_orows_weight_first(b, 1)
 * (default 0; any other value MRK_E_INVAL).  It takes effect with the next submit, and all rows of a submit -- the standing
 * order-row destination's, mrk_batch_export_orows' after the wait, the row repaired by an overflow rerun -- follow the setting that
 * stood when it was submitted.  With it off, and in narrow and wide rows whatever it says, a weight-first query leaves with
 * MRK_ROW_DECLINED, no keys and spec word 0.
 * ---------------------------------------------------------------------------------- */
#define MRK_OROW_WORDS (MRK_ROW_WORDS + MRK_MAX_K + 1)
int mrk_batch_export_orows(mrk_batch* b, uint64_t* orows_dst);
int mrk_batch_set_orows_dst(mrk_batch* b, uint64_t* orows_dst);
int mrk_batch_orows_weight_first(mrk_batch* b, int on);
int mrk_topk_merge_orows(mrk_ctx* ctx, const uint64_t* orows_all, uint32_t n_lists, uint32_t n_queries, uint32_t k, uint64_t* out_orows);
int mrk_topk_merge_orows_async(mrk_ctx* ctx, const uint64_t* orows_all, uint32_t n_lists, uint32_t n_queries, uint32_t k,
                               uint64_t* out_orows, void* wait_event, uint32_t slot);
int mrk_topk_merge_orows_part(mrk_ctx* ctx, const uint64_t* orows_recv, uint32_t n_lists, uint32_t list_stride, uint32_t first, uint32_t count,
                              uint32_t k, uint64_t* out_orows);
int mrk_shard_exchange_orows(mrk_ctx* ctx, mrk_batch* batch, const uint64_t* orows, uint32_t n_queries, uint32_t k, uint64_t* out_orows,
                             uint32_t slot);
/* host only: the value behind a 64-bit mapped key of a row with this order spec word, in mrk_result.order_key's format: the raw
   int64, or raw0 << 32 | raw1 (a sort spec: raw0 << 32).  A float's -0.0 reads +0.0.  A weight-first spec unmaps its parts as the
   same spec without bit 3 does; one without parts unmaps to 0. */
uint64_t mrk_order_unmap_key(uint64_t spec_word, uint64_t mapped);

/* ------------------------------------------------------------------------------------
 * Group rows: grouped queries (mrk_group) across segments and shards.  The yardstick is ONE grouping sorter fed with the matches
 * of all segments, as the reference searches the chunks of one index: RtIndex_c::MultiQuery hands the same sorters to every disk
 * chunk (QueryDiskChunks, sphinxrt.cpp:6018-6077: each chunk's MultiQuery pushes into dSorters, :6541) and then to every RAM
 * segment (PerformFullTextSearch, :6302-6346: ARRAY_FOREACH over dRamChunks into the same dSorters, :6431).  Its distributed
 * master / agent setups are NOT the yardstick: an agent returns max_matches groups only, so their counts are approximate.
 * The three top-K merges above take the best K of a union of entries; groups need their counts ADDED per key and the better head
 * kept, and a group outside a shard's own top K may be inside the merged top K.  So a group row carries ALL groups of its list.
 * One row of MRK_GROW_WORDS u64 per query, G = MRK_GROW_GROUPS = 4 * MRK_MAX_K:
 *   [0 .. G-1]        the head keys of the row's groups, in GROUP ORDER, best first, zero past the count
 *   [G] [G+1]         number of entries | total_found with MRK_ROW_RERUN / MRK_ROW_DECLINED, as in every row
 *   [G+2 .. 2G+1]     per entry: the group value in the high dword, @count in the low dword; zero past the count
 *   [2G+2]            the group spec word: 0 = a relevance query; else bit 0 grouped | bits 1-2 sort_by (MRK_GROUPSORT_*) |
 *                     bit 3 desc | bits 8-13 bit_count | bits 16-26 max_matches, every other bit zero -- what every merger needs
 *                     to apply the same 4 * max_matches limit and take the same first max_matches, nothing of where a segment
 *                     stores the column
 * A grouped query's row holds all its groups (at most 4 * max_matches), sorted; the first min(n, max_matches) entries are what
 * mrk_result gives.  total_found is the number of groups.  A relevance query travels in group rows too, so a mixed batch needs one
 * exchange: its top-K keys in words [0, MRK_MAX_K), a zero plane and spec 0.  A mrk_query.sort / .order query leaves with
 * MRK_ROW_DECLINED, no keys and spec 0, and so does a grouped query that was declined, at plan time or while it ran (more than
 * 4 * max_matches groups).
 * The merge, per group value: @count = the sum of the lists' counts, head = the largest head key (weight DESC, global rowid ASC),
 * the groups ordered as the spec says, total_found = the number of distinct merged groups (NOT the sum of the lists' totals).  Both
 * steps are associative and commutative: a staged merge (segments, then shards) gives the same words as one merge of all lists,
 * and a decline anywhere stays one.  A spec-0 query merges exactly as mrk_topk_merge_rows does (words [0, MRK_MAX_K), [G] and [G+1]
 * equal that merge's keys, count and total word).  For a grouped query:
 *   any list with MRK_ROW_RERUN            -> MRK_ROW_RERUN, no entries
 *   any list with MRK_ROW_DECLINED, answering lists whose spec words differ in any bit, a grouped list next to a spec-0 one, more
 *   than 4 * max_matches merged groups, a sum of counts above 2^32 - 1 (never wrapped or saturated)
 *                                          -> MRK_ROW_DECLINED, no entries, the spec word of the first answering list
 * The spec word is elected among the answering lists: every list but one that comes MRK_ROW_DECLINED under spec word 0 (a shard
 * whose planner declined the query; such a list's spec is not compared, so the merged row does not depend on which list declined).
 * A list declined under its own spec word -- over the limit while it ran, or the merged row of lists that were -- keeps its say.
 * A list whose entry count exceeds G, or whose spec word is neither 0 nor a grouped spec as above, is read as a list with
 * MRK_ROW_DECLINED, no entries and spec 0: hostile rows never make the merge read or write out of bounds.
 * k: the largest max_matches of the call's queries; it sizes the merge's tables (a context-owned scratch arena) and is the k of
 * the spec-0 merge.  A grouped row whose max_matches exceeds k merges to MRK_ROW_DECLINED.  At most 8 lists.
 * mrk_batch_export_grows is called after mrk_batch_wait (the batch's group tables stay alive until its next grouped submit); a
 * query rerun after a match-queue overflow leaves with its repaired groups.  There is no standing destination for group rows and
 * ShardMerger does not carry them: both are left.  Group functions other than one integer attribute are left too.
 * ---------------------------------------------------------------------------------- */
#define MRK_GROW_GROUPS (4 * MRK_MAX_K)
#define MRK_GROW_WORDS (2 * MRK_GROW_GROUPS + 3)
int mrk_batch_export_grows(mrk_batch* b, uint64_t* grows_dst);
int mrk_topk_merge_grows(mrk_ctx* ctx, const uint64_t* grows_all, uint32_t n_lists, uint32_t n_queries, uint32_t k, uint64_t* out_grows);
int mrk_topk_merge_grows_async(mrk_ctx* ctx, const uint64_t* grows_all, uint32_t n_lists, uint32_t n_queries, uint32_t k,
                               uint64_t* out_grows, void* wait_event, uint32_t slot);
int mrk_topk_merge_grows_part(mrk_ctx* ctx, const uint64_t* grows_recv, uint32_t n_lists, uint32_t list_stride, uint32_t first, uint32_t count,
                              uint32_t k, uint64_t* out_grows);
int mrk_shard_exchange_grows(mrk_ctx* ctx, mrk_batch* batch, const uint64_t* grows, uint32_t n_queries, uint32_t k, uint64_t* out_grows,
                             uint32_t slot);
/* host only: the group spec word of a query (0 where the fields are no valid spec) */
uint64_t mrk_group_spec_word(uint32_t sort_by, uint32_t desc, uint32_t bit_count, uint32_t max_matches);

/* ------------------------------------------------------------------------------------
 * Aggregate rows: grouped queries WITH their aggregates (mrk_aggrs) across segments and shards.  The yardstick is the group rows':
 * ONE grouping sorter fed with the matches of all segments (the citations above), not the reference's master / agent merge.  The
 * accumulators are adds and maxima, associative and commutative as the counts and heads are, so a group row's contract carries
 * over word for word; the row grows by MRK_MAX_AGGRS planes and a second spec word.
 * One row of MRK_AROW_WORDS = 6 G + 4 u64 per query, G = MRK_GROW_GROUPS:
 *   [0 .. 2G+1]         head keys | count | total word | group value << 32 | @count: as in a group row
 *   [2G+2 + a*G + i]    aggregate a (< MRK_MAX_AGGRS) of entry i: the VALUE, exactly as mrk_batch_result_aggrs gives it -- a 32-bit
 *                       result zero-extended, a 64-bit one the integer's bits.  Zero past the count, for a >= n and in a row
 *                       without aggregates
 *   [6G+2]              the group spec word, unchanged
 *   [6G+3]              the aggregate spec word: 0 = no aggregates; else bit 0 set | bits 1-3 n (1..4) | bits 4-6 1 + order_by (0 =
 *                       none) | for aggregate a, bits 8+4a .. 11+4a: func (MRK_AGGR_*, the low 2 bits) | bit 2 a signed 64-bit
 *                       source | bit 3 widened; every other bit zero.  Nothing of where a segment stores the column.
 * What travels: a grouped query with aggregates, with all its groups; a grouped query without, with zero planes and aggregate spec
 * 0 (its words [0, 2G+2) and its group spec word equal its group row); a relevance query as in group rows (keys in [0, MRK_MAX_K),
 * both specs 0).  A mrk_query.sort / .order query and one the planner declined leave MRK_ROW_DECLINED under spec words 0; a grouped
 * query declined while it ran (more than 4 * max_matches groups) leaves MRK_ROW_DECLINED, one the scan flagged MRK_ROW_RERUN, both
 * without entries under their own two spec words.  The other four row kinds decline a query with aggregates.
 * The merge: the group spec is elected as in group rows, and the aggregate spec words of the lists that have a say must be equal in
 * every bit -- "grouped with aggregates" next to "grouped without" included -- or the merged row is MRK_ROW_DECLINED without
 * entries under the first answering list's two spec words.  MRK_ROW_RERUN, a decline in any list, the 4 * max_matches limit over
 * all lists, a count sum past 2^32 - 1 and max_matches > k: as in group rows.  Per group value counts add, the larger head stays,
 * SUM adds (modulo 2^32 for a 32-bit result, modulo 2^64 otherwise), MIN / MAX compare unsigned for INT sources (widened or not) and
 * signed for INT64 sources.  The groups are ordered by the group spec, or by the ordering aggregate's MERGED 32-bit value in the
 * group spec's direction, then by head rowid ascending; total_found = the number of merged groups.  A staged merge equals a
 * one-step merge word for word; a spec-0 query merges exactly as mrk_topk_merge_grows merges it.
 * Hostile lists read as MRK_ROW_DECLINED, no entries, both spec words 0: an entry count above G, a group spec that does not unpack,
 * an aggregate spec with a stray bit, n out of range, func 0 inside n or a nonzero field beyond it, both width bits, an order that
 * names a 64-bit result or an index >= n, an order next to a group spec whose sort_by is not MRK_GROUPSORT_KEY, or a nonzero
 * aggregate spec over group spec 0.
 * Limits shared with the group rows: at most 8 lists; k = the largest max_matches of the call (it sizes the context's scratch arena,
 * here with room for MRK_MAX_AGGRS planes per table); the merge is synchronous on the merge stream (_async: behind it);
 * mrk_batch_export_arows is called after mrk_batch_wait, and a rerun query leaves with its repaired groups and aggregates.
 * Left, as for group rows: there is no standing destination for aggregate rows, and ShardMerger does not carry them.  AVG and
 * float sources are not offered (mrk_aggrs above).
 * ---------------------------------------------------------------------------------- */
#define MRK_AROW_WORDS (6 * MRK_GROW_GROUPS + 4)
int mrk_batch_export_arows(mrk_batch* b, uint64_t* arows_dst);
int mrk_topk_merge_arows(mrk_ctx* ctx, const uint64_t* arows_all, uint32_t n_lists, uint32_t n_queries, uint32_t k, uint64_t* out_arows);
int mrk_topk_merge_arows_async(mrk_ctx* ctx, const uint64_t* arows_all, uint32_t n_lists, uint32_t n_queries, uint32_t k,
                               uint64_t* out_arows, void* wait_event, uint32_t slot);
int mrk_topk_merge_arows_part(mrk_ctx* ctx, const uint64_t* arows_recv, uint32_t n_lists, uint32_t list_stride, uint32_t first, uint32_t count,
                              uint32_t k, uint64_t* out_arows);
int mrk_shard_exchange_arows(mrk_ctx* ctx, mrk_batch* batch, const uint64_t* arows, uint32_t n_queries, uint32_t k, uint64_t* out_arows,
                             uint32_t slot);
/* host only: the aggregate spec word of a query's aggregates next to a group with this sort_by (0 where the fields are no valid
   spec: NULL, n or order_by out of range, an unknown func, kind or flag, WIDEN on an INT64 source, a 64-bit order, an order next to
   another sort_by) */
uint64_t mrk_aggr_spec_word(const mrk_aggrs* aggrs, uint32_t group_sort_by);

/* merge n_lists sorted partial top-K lists per query (device pointers; relevance order only):
   in_keys[(l*n_queries + q)*MRK_MAX_K + i], in_counts[l*n_queries + q] -> out_keys[q*MRK_MAX_K + i],
   out_counts[q].  Order: weight desc, global docid asc. Synchronous on the ctx stream. */
int mrk_topk_merge(mrk_ctx* ctx, const uint64_t* in_keys, const uint32_t* in_counts, uint32_t n_lists,
                   uint32_t n_queries, uint32_t k, uint64_t* out_keys, uint32_t* out_counts);

/* IDF exactly as sphCreateRanker computes it (host libm logf) */
float mrk_idf(int64_t term_docs, int64_t total_docs, int plain_idf, int normalized, int n_qwords, float boost);

/* ------------------------------------------------------------------------------------
 * Host-side index construction (format writer + synthetic corpus); no GPU involved.
 * Writer follows CSphHitBuilder (sphinx.cpp:8378-8719) byte for byte.
 * ---------------------------------------------------------------------------------- */
typedef struct mrk_host_index mrk_host_index;

/* hits sorted by (wordid, rowid, hitpos); wordid = term id + 1 */
int mrk_index_from_hits(const uint64_t* wordid, const uint32_t* rowid, const uint32_t* hitpos, uint64_t n,
                        uint32_t n_terms, uint32_t skiplist_block_size, uint32_t hit_format, mrk_host_index** out);

typedef struct {
  uint64_t seed;
  uint64_t n_docs;          /* docs in this segment (rowids 0..n_docs-1) */
  uint64_t rowid_base;      /* global rowid of the segment's rowid 0: postings are a function of (seed, term, global rowid),
                               so shards [base, base + n_docs) are slices of the one corpus */
  const double* term_prob;  /* document probability of each generated term */
  uint32_t n_terms;
  uint32_t n_fields;        /* hits fall into field 0 with prob title_frac, else uniformly in 1..n_fields-1 */
  double title_frac;
  uint32_t max_pos;         /* positions uniform in [1, max_pos] */
  uint32_t skiplist_block_size;
  uint32_t hit_format;
  uint32_t end_markers;     /* field-end bits: 0 none; 1 on each word's own last hit per field (two words at one position may differ in it);
                               2 on the hit at the field's last POSITION in that doc, whatever the word -- what the reference's indexer writes */
  uint32_t n_threads;       /* 0 = hardware concurrency */
} mrk_synth_params;

int mrk_synth_generate(const mrk_synth_params* p, mrk_host_index** out);
void mrk_host_index_free(mrk_host_index* h);
/* buffers have 64 zero bytes of slack after *len */
const uint8_t* mrk_host_index_spd(const mrk_host_index* h, uint64_t* len);
const uint8_t* mrk_host_index_spp(const mrk_host_index* h, uint64_t* len);
const uint8_t* mrk_host_index_spe(const mrk_host_index* h, uint64_t* len);
const mrk_dict_entry* mrk_host_index_dict(const mrk_host_index* h, uint32_t* n_terms);

/* Accounting aid for the roofline figures; not on the query path.  For each keyword pair
   (pairs[2i], pairs[2i+1]): common docs, each keyword's doc count, and the distinct 128-byte lines of each keyword's packed
   tf / field words (64 words per 128-doc block, in doclist order) that the common docs touch -- what the two-bitmap AND
   kernel's gathers have to fetch, instead of "every tf / field word of both doclists" -- and the distinct 128-doc
   blocks touched (= 128-byte lines of the one-byte-per-doc "attr_nibbles" plane); lines128s_*: the same count for the
   slot-ordered two-byte plane ("attr_seq": 64 consecutive docs per 128-byte line), which is what the kernel gathers from by
   default. */
typedef struct {
  uint64_t matches, docs_a, docs_b, lines128_a, lines128_b, blocks_a, blocks_b, lines128s_a, lines128s_b;
} mrk_pair_stats;
int mrk_host_index_pair_stats(const mrk_host_index* h, uint32_t hit_format, const uint32_t* pairs, uint32_t n_pairs,
                              uint32_t n_threads, mrk_pair_stats* out);

/* ------------------------------------------------------------------------------------
 * Real index ingestion: the files a Manticore 3.x indexer / RT disk chunk wrote,
 * format versions 54..62, read from disk into the same host-side object.  Replaces CSphIndex_VLN::LoadHeader
 * (sphinx.cpp:13252-13388), CWordlist::Preread + the dictionary block readers (indexformat.cpp:279-344, 425-470,
 * 641-691) and DeadRowMap_Disk_c (killlist.cpp:171-184) for what the match -> rank -> top-K path needs.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  uint32_t version;             /* .sph format version (54..62) */
  uint32_t n_fields, n_attrs;   /* schema */
  uint32_t skiplist_block_size; /* 128 before v56, else the stored setting */
  uint32_t hit_format;          /* MRK_HITFMT_* (ESphHitFormat) */
  uint32_t hitless;             /* ESphHitless; only 0 (none) can be searched here */
  uint32_t word_dict;           /* 1 = dict=keywords, 0 = dict=crc */
  uint32_t min_prefix_len, min_infix_len;
  uint32_t index_sp, index_field_lens;
  uint32_t n_checkpoints;
  uint64_t total_docs, total_bytes; /* m_tStats */
  uint64_t n_dead;                  /* bits set in the .spm dead-row map */
} mrk_index_info;

/* path_prefix + ".sph" / ".spi" / ".spd" / ".spp" / ".spe" (/ ".spm", optional).  Term ids of the result are the
   dictionary's entries in file order (sorted by keyword for dict=keywords, by word id for dict=crc). */
int mrk_index_open(const char* path_prefix, mrk_host_index** out);
int mrk_host_index_info(const mrk_host_index* h, mrk_index_info* out); /* MRK_E_INVAL unless opened from files */
const char* mrk_host_index_field_name(const mrk_host_index* h, uint32_t field);
/* dict=keywords: term id of a keyword (sphDictCmpStrictly order, sphinxint.h), -1 = not in the dictionary */
int32_t mrk_host_index_find_word(const mrk_host_index* h, const char* word, int32_t len);
const char* mrk_host_index_word(const mrk_host_index* h, uint32_t term_id, uint32_t* len);
/* dict=crc: term id of a word id, -1 = absent */
int32_t mrk_host_index_find_wordid(const mrk_host_index* h, uint64_t wordid);
/* Schema attributes as the header lists them (CSphColumnInfo: name, ESphAttr type, locator) and the row-wise storage of
   the .spa file: the first n_rows (= m_iDocinfo) rows of stride dwords -- what mrk_segment_set_attrs takes; the min-max
   index that follows them in the file is not used.  NULL / 0 when the index has no .spa (no attributes but the id). */
typedef struct {
  const char* name;
  uint32_t type;       /* ESphAttr (sphinx.h): 1 = uint, 2 = timestamp, 4 = bool, 5 = float, 6 = bigint, ... */
  int32_t bit_offset;  /* CSphAttrLocator::m_iBitOffset; < 0 for blob-stored attributes */
  int32_t bit_count;
} mrk_attr_info;
int mrk_host_index_attr(const mrk_host_index* h, uint32_t i, mrk_attr_info* out); /* i < mrk_index_info.n_attrs */
const uint32_t* mrk_host_index_attr_rows(const mrk_host_index* h, uint32_t* stride_dwords, uint64_t* n_rows);
/* .spm bitmap (bit rowid & 31 of word rowid >> 5), as mrk_segment_set_dead_rows takes it; NULL = no map */
const uint32_t* mrk_host_index_dead_rows(const mrk_host_index* h, uint64_t* n_rows);
/* the blob pool (.spb file as it is / an RT segment's m_dBlobs), NULL = none; n_blob_attrs = the schema's blob-stored attributes
   (strings, MVAs, JSON: those with bit_count 0, in schema order = their blob attribute ids) */
const uint8_t* mrk_host_index_blobs(const mrk_host_index* h, uint64_t* len, uint32_t* n_blob_attrs);

/* ---- RT index RAM chunk (host only) ---------------------------------------------------------------------------------------
   path_prefix + ".meta" / ".ram" as RtIndex_c::SaveMeta / SaveRamChunk write them (sphinxrt.cpp:3560-3640, 4034-4103; meta
   v.14-18).  Each RAM segment (RtSegment_t: its own dictionary, doclists and hitlists in the RT codecs, sphinxrt.cpp:390-640,
   rows, dead-row map) comes back as a mrk_host_index in the disk format -- decoded and re-emitted, so that an RT segment is
   one more mrk_segment for mrk_topk_merge; rowids are segment-local as in the reference.  Stepped over: stored fields (the docstore); not read: the
   blob pool; declined: hitless words.  mrk_rt_ram_take hands segment i to the caller (free it with mrk_host_index_free). */
typedef struct mrk_rt_ram mrk_rt_ram;
int mrk_rt_ram_open(const char* path_prefix, mrk_rt_ram** out);
uint32_t mrk_rt_ram_segments(const mrk_rt_ram* rt);
int mrk_rt_ram_take(mrk_rt_ram* rt, uint32_t i, mrk_host_index** out);
void mrk_rt_ram_free(mrk_rt_ram* rt);
/* A LIVE RAM segment handed over in memory (round 3): the byte vectors of an RtSegment_t (sphinxrt.h:140-149) -- m_dWords (the
   dictionary: keywords front-coded / word-id deltas, restarted every words_checkpoint entries), m_dDocs, m_dHits in the RT codecs --
   decoded and re-emitted in the disk format exactly as mrk_rt_ram_open does for the segments of a .ram file (same code).  The
   result is an ordinary mrk_host_index (mrk_host_index_spd / _dict / _find_word ...): mrk_segment_create it once when the segment
   appears (RAM segments are immutable once committed), hand its dead-row map and attribute rows over with
   mrk_segment_set_dead_rows / _set_attrs, and let the ranker binding pick it when RtIndex_c rebinds the ranker to that segment
   (ISphRanker::Reset, sphinxrt.cpp:6313-6314).  rows = RtSegment_t::m_uRows; words_checkpoint = RtIndex_c::m_iWordsCheckpoint. */
typedef struct {
  const uint8_t* words;
  uint64_t words_len;
  const uint8_t* docs;
  uint64_t docs_len;
  const uint8_t* hits;
  uint64_t hits_len;
  uint32_t rows;
  uint32_t word_dict;        /* 1 = dict=keywords, 0 = dict=crc */
  uint32_t words_checkpoint;
  uint32_t skiplist_block_size; /* of the re-encoded doclists; 0 = 128 */
  uint32_t hit_format;       /* MRK_HITFMT_* of the re-encoded doclists */
  uint32_t n_fields;
} mrk_rt_segment_desc;
int mrk_rt_segment_open(const mrk_rt_segment_desc* desc, mrk_host_index** out);

/* ---- query text -> tree (host only) ------------------------------------------------------------------------------------
   The caller side of the path: the extended query syntax (sphParseExtendedQuery: sphinxquery.y:57-125 grammar; the lexer
   XQParser_t::GetToken, sphinxquery.cpp:1201-1553; AddKeyword / AddOp, :1600-1678; FixupNots, :499-562) restated for the
   operators this library evaluates:  a b   a | b   a MAYBE b   -a  !a   ( )   "a b"   "a b"~N   "a b c"/N   "a b c"/0.5
   a << b   a NEAR/N b   a NOTNEAR/N b   a SENTENCE b   a PARAGRAPH b   @field  @(f1,f2)  @!field  @!(f1,f2)  @*  @field[N]  @@relaxed   ^a  a$  =a  a^1.5
   and '*' inside a phrase.  The result is the flat mrk_node[] + children[] form mrk_query takes (post-order, root last):
   query positions (atom_pos) in textual order, field limits as masks, NOT folded into ANDNOT, one-word phrases folded to
   their word, fractional quorum thresholds resolved against the word count.  'a SENTENCE b' / 'a PARAGRAPH b' come back as
   MRK_OP_SENTENCE / _PARAGRAPH nodes whose keyword text (mrk_parsed_keyword) is the boundary word "\3sentence" /
   "\3paragraph" for the dictionary lookup.  ZONE / ZONESPAN are not recognised (their capitals read as keywords).
   Tokenizing is ASCII [A-Za-z0-9_] + bytes >= 0x80, lower-casing ASCII only -- a host with a charset_table, morphology,
   stopwords or wordforms runs its own tokenizer / dictionary over the keywords' text; what this entry point fixes is the
   grammar.  Words shorter than min_word_len (code points) are dropped and keep their position (overshort_step = 1).
   field_names[i] is the name of full-text field i (bit i of a field mask).  Keywords come back as text
   (mrk_parsed_keyword); mrk_parsed_resolve fills term_id from a dict=keywords dictionary.  A syntax error returns
   MRK_E_INVAL with the reason in mrk_last_error() (the reference's "query error: ..."). */
typedef struct mrk_parsed_query mrk_parsed_query;
int mrk_query_parse(const char* text, const char* const* field_names, uint32_t n_fields, uint32_t min_word_len,
                    mrk_parsed_query** out);
/* sphTransformExtendedQuery (sphinx.cpp:15345-15359), the part every query goes through between the parser and the ranker:
   a quorum with threshold 1 -> the OR of its words (TransformQuorum); AND groups among a NEAR node's operands are replaced by their
   children, '(a b c) NEAR/N d' -> 'a NEAR/N b NEAR/N c NEAR/N d' (TransformNear).  In place.  Not restated: TransformBigrams (needs
   a bigram_index index) and the boolean simplifier (sphOptimizeBoolean: OPTION boolean_simplify, off by default). */
int mrk_parsed_transform(mrk_parsed_query* q);
void mrk_parsed_free(mrk_parsed_query* q);
int32_t mrk_parsed_n_nodes(const mrk_parsed_query* q);
int32_t mrk_parsed_root(const mrk_parsed_query* q); /* -1: the query holds no keyword (matches nothing) */
const mrk_node* mrk_parsed_nodes(const mrk_parsed_query* q);
const int32_t* mrk_parsed_children(const mrk_parsed_query* q, int32_t* n);
const char* mrk_parsed_keyword(const mrk_parsed_query* q, int32_t node); /* "" for operator nodes */
int mrk_parsed_resolve(mrk_parsed_query* q, const mrk_host_index* h);

#ifdef __cplusplus
}
#endif
#endif /* MRK_H */
