// qe_kernels.h -- host-callable launchers of the precompiled (AOT) gfx950 kernels.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include "../../include/qe_hip.h"

namespace qe {

// synthetic column generator; data/validity are device pointers
void launch_generate(hipStream_t s, const qe_gen_spec &spec, uint64_t seed, int64_t row_begin, int64_t nrows,
                     void *data, uint64_t *validity);
// bytes (0/1 per row) -> bitmap words (row i = word i>>6 bit i&63)
void launch_pack_bytes(hipStream_t s, const uint8_t *bytes, int64_t n, uint64_t *words);
// plain streaming read of nbytes (16 B per lane), result folded into sink[0] so nothing is elided
void launch_stream_read(hipStream_t s, const void *src, int64_t nbytes, unsigned long long *sink, int wgs_per_cu = 8);

// read stream + a trickle of writes (one 512-byte block per wave every `write_every` read iterations of 8 KiB)
void launch_stream_read_write(hipStream_t s, const void *src, int64_t nbytes, unsigned long long *sink, void *dst,
                              int64_t dst_bytes, int write_every, int window_period, int window_len, int blocks_per_event);

// hashed group-by: fill a table of nentries entries with the per-word pattern of an empty entry; copy the entries in use
// (state word == 2) to a dense array, *counter = how many
struct HtInit {
    int words;
    unsigned long long word[40];
};
void launch_ht_init(hipStream_t s, unsigned long long *tab, int64_t nentries, const HtInit &init);
void launch_ht_collect(hipStream_t s, const unsigned long long *tab, int64_t nentries, int words, unsigned long long *dense,
                       unsigned int *counter);

// ---- groups of a hashed GROUP BY finished on the device (qe_kernels.hip) ----
// entries: m x `words` u64 {state, null bits of the keys, key words.., first row, (count, acc) per aggregate}
// sort keys: keys[i] = first row of entry i, rows[i] = i; after the radix passes rows[] lists the entries in insertion order
void launch_group_sort_keys(hipStream_t s, const unsigned long long *entries, int words, int first_row_word, int64_t m,
                            unsigned long long *keys, uint32_t *rows);
struct GroupFinishArgs {
    const unsigned long long *entries;
    const unsigned int *rows;        // entry of result row j
    long long m;
    int words, nkeys, nagg;
    int key_type[4];                 // QE_* of the key columns
    void *key_data[4];               // DOUBLE / INT64: u64[m]; INT32 / STRING: i32[m]; BOOLEAN: bitmap words
    unsigned long long *key_valid[4];
    int agg_fn[8], cnt_src[8];       // QE_AGG_*, and which aggregate's counter says whether aggregate i saw a value
    double *agg_data[8];
    unsigned long long *agg_valid[8];
    unsigned int *flags;             // [k] = 1: some group has a NULL in key k; [4 + i]: aggregate i is NULL somewhere
};
void launch_group_finish(hipStream_t s, const GroupFinishArgs &a);

// ---- ORDER BY (qe_sort.hip) ----
// keys[i] = order-preserving u64 image of row i of the key column (0 under a NULL), rows[i] = i
struct SortKeyArgs {
    int type;                       // QE_* of the key column
    const void *data;
    const unsigned long long *validity;
    const int *ranks;               // QE_STRING: compareTo rank per dictionary code
    int nranks;
    long long n;
    unsigned long long *keys;
    unsigned int *rows;             // rows[i] = i is written when `perm` is null (may be null: images only)
    const unsigned int *perm;       // not null: keys[j] = image of row perm[j] (a later key of a multi-key sort)
    int descending;                 // 1: the complement of the image (reversed comparator; NULL = all ones)
};
void launch_sort_keys(hipStream_t s, const SortKeyArgs &a);
// or_and[0] |= every key, or_and[1] &= every key (caller initialises to {0, ~0})
void launch_key_bits(hipStream_t s, const unsigned long long *keys, int64_t n, unsigned long long *or_and);
// one stable LSD radix pass over the 4 key bits at `shift` (shift == 64: over the validity bit of each element's row, NULL
// first; shift == 65: NULL last, for a descending key); hist: 16 * ceil(n / 1024) u32 of scratch
void launch_radix_pass(hipStream_t s, const unsigned long long *keys, const uint32_t *rows, const uint64_t *validity, int64_t n, int shift,
                       uint32_t *hist, unsigned long long *keys_out, uint32_t *rows_out);
// ORDER BY .. LIMIT k: radix select over the first key's images (8 bits per pass, most significant first).  The state lives
// in device memory and is zero-initialised by the caller except `remaining` = k; launch_select_pass = histogram of the digit
// at `shift` among the rows that match the prefix + the one-wave step that extends the prefix (and sets `done` once at most
// stop_cap rows are <= the prefix).  Candidates = rows whose masked image is <= the prefix, ties of the k-th row included.
struct SelectState {
    unsigned long long prefix, mask, remaining, below;
    unsigned int bucket, done, passes, pad;
    unsigned int hist[256];
};
void launch_select_pass(hipStream_t s, const unsigned long long *keys, int64_t n, int shift, SelectState *state, unsigned long long stop_cap);
int64_t select_compact_blocks(int64_t n);   // blocks of the two kernels below = entries of counts / offsets
void launch_select_count(hipStream_t s, const unsigned long long *keys, int64_t n, const SelectState *state, uint32_t *counts);
// row ids of the candidates in row order; offsets = exclusive scan of counts; at most `capacity` ids are written
void launch_select_compact(hipStream_t s, const unsigned long long *keys, int64_t n, const SelectState *state, const uint32_t *counts,
                           const uint32_t *offsets, uint32_t *rows_out, int64_t capacity);

// ---- hash equi-join (qe_join.hip) ----
// the key columns of one side; the image of a key column is the u64 two equal values share
struct JoinKeyCols {
    int nkeys;
    int type[4];                            // QE_* of the key columns
    const void *data[4];
    const unsigned long long *validity[4];  // or null
    const int *remap[4];                    // QE_STRING: code -> canonical code in the BUILD dictionary (-1: not there); null = the code itself
    int ncodes[4];                          // QE_STRING: entries of the column's dictionary (a code outside matches nothing)
};
// build: hash[i], rows[i] = i and img[k][i] of every row, bit i of valid_words = the key holds no NULL, *nvalid += such rows
struct JoinBuildArgs {
    JoinKeyCols kc;
    long long n;
    unsigned long long mask;                // bits of the hash that are kept ($QE_JOIN_HASH_BITS)
    unsigned long long *hash;
    unsigned int *rows;
    unsigned long long *img[4];
    unsigned long long *valid_words;
    unsigned long long *nvalid;
};
void launch_join_build_keys(hipStream_t s, const JoinBuildArgs &a);
// dir[b] = first of the m sorted entries whose top dbits hash bits are >= b; 2^dbits + 1 entries
void launch_join_directory(hipStream_t s, const unsigned long long *sorted_hash, int64_t m, int dbits, uint32_t *dir);
// the table as the probe sees it: entries sorted by bucket, inside a bucket in build-row order
struct JoinTableView {
    const unsigned int *dir;
    const unsigned int *rows;               // build row of sorted entry s
    const unsigned long long *img[4];       // its key images
    int dbits, nkeys;
    unsigned long long mask;
};
struct JoinProbeArgs {
    JoinKeyCols kc;
    JoinTableView t;
    long long n;                            // probe rows
    int join_type;                          // QE_JOIN_*
    unsigned int *cnt;                      // output rows of probe row i
    unsigned int *first;                    // sorted entry of its first match (0xFFFFFFFF: none); null for SEMI / ANTI
    unsigned long long *blocksum;           // per block of 256 probe rows: pass 1 writes the sum, the carry scan (qe_scan.h) the offset
    unsigned int *longest;                  // max over the probe rows of the entries one row walked
    unsigned long long total;               // pass 2: pairs the lists hold
    unsigned int *prow_out, *brow_out;      // pass 2: the pairs (brow_out null for SEMI / ANTI; build row 0xFFFFFFFF = none)
    unsigned long long *matched;            // RIGHT / FULL (join_type is then the head's, INNER / LEFT): pass 1 sets bit r of this
                                            // zeroed bitmap over BUILD ROWS for every build row r it finds equal; null otherwise,
                                            // and pass 1 is then the kernel without the marks
};
int64_t join_probe_blocks(int64_t n);       // entries of blocksum
void launch_join_count(hipStream_t s, const JoinProbeArgs &a);
void launch_join_write(hipStream_t s, const JoinProbeArgs &a);
// RIGHT / FULL of the hash join and the range join: the `matched` bitmap over the n rows of the build / right side becomes the
// bitmap of the rows NOBODY matched -- every word complemented, the bits past row n cleared; ceil(n / 64) whole words
void launch_join_unmatched(hipStream_t s, unsigned long long *words, int64_t n);

// ---- window functions over a sorted result (qe_window.hip) ----
constexpr int kWinTileRows = 2048;    // T: rows of one scan tile (4 waves x 8 words of 64 rows)
constexpr int kWinTripTiles = 1024;   // tile aggregates one trip of the one-workgroup scan holds
// Boundary flags of the sorted rows: bit j of pstart = row j starts a partition (row 0, or it differs from row j - 1 in the
// sort image or the validity of one of the first npart keys), bit j of peer = it starts a partition or differs on a later
// key.  perm[j] = source row that stands at j (null: j itself).  *npartitions += set bits of pstart.
struct WinFlagArgs {
    int nkeys, npart;
    int type[8];
    const void *data[8];
    const unsigned long long *validity[8];
    const int *ranks[8];                    // QE_STRING: compareTo rank per dictionary code (the sort's table)
    int nranks[8];
    const unsigned int *perm;
    long long n;
    unsigned long long *pstart, *peer;      // ceil(n / 64) words each, whole words are written
    unsigned long long *npartitions;
};
void launch_win_flags(hipStream_t s, const WinFlagArgs &a);
// One segmented inclusive scan over the n rows, restarted at every set bit of pstart, in three fixed-shape steps: per-tile
// reduce, one workgroup over the tile aggregates (kWinTripTiles per trip), per-tile downsweep.  reverse: the scan runs from
// row n - 1 down and restarts after every row that ENDS a partition (the next row's pstart bit, or row n - 1); block > 0: it
// also restarts at every row j with j % block == 0 (reverse: after every row with j % block == block - 1).
enum { QE_WSCAN_SUM = 0, QE_WSCAN_MIN = 1, QE_WSCAN_MAX = 2, QE_WSCAN_INDEX = 3 };
enum { QE_WOUT_SUM = 0, QE_WOUT_MINMAX = 1, QE_WOUT_AVG = 2, QE_WOUT_COUNT = 3, QE_WOUT_COUNT_I64 = 4, QE_WOUT_INDEX = 5, QE_WOUT_ITEM = 6 };
struct WinScanArgs {
    int op;                                 // QE_WSCAN_*
    int out_mode;                           // QE_WOUT_*
    int type;                               // QE_DOUBLE / QE_INT64 / QE_INT32 of data
    const void *data;                       // null: only the count of valid rows is scanned
    const unsigned long long *validity;     // null: every row valid.  QE_WSCAN_INDEX: the bitmap whose last set bit at or before each row is wanted
                                            // (reverse: a partition-start bitmap; the first partition END at or after each row is wanted)
    const unsigned long long *pstart;       // null: one segment
    int reverse;                            // 1: from row n - 1 down
    long long block;                        // > 0 (and < 2^32): extra restarts at the edges of blocks of this many rows
    long long n, ntiles;
    double *tile_v, *carry_v;               // ntiles each: the tile aggregates, and what the scan over them carries into each tile
    unsigned int *tile_c, *tile_f, *carry_c;
    void *out;                              // f64 (SUM, MINMAX, AVG, COUNT, ITEM), i64 (COUNT_I64) or u32 (INDEX) per row
    unsigned int *out_c;                    // QE_WOUT_ITEM: the scanned pair {out[j], out_c[j]} = {value, valid values} as it stands
    unsigned long long *out_valid;          // SUM, MINMAX, AVG: bit j = a valid value has been seen in the partition up to row j
};
void launch_win_scan(hipStream_t s, const WinScanArgs &a);
// out[j] = (first ? first[j] : j) - start[j] + 1: ROW_NUMBER (first null) and RANK (first = index of the first peer)
void launch_win_rank(hipStream_t s, const uint32_t *start, const uint32_t *first, int64_t n, int64_t *out);
// A framed aggregate, one elementwise pass: the frame of row j is [lo, hi] = [preceding < 0 ? start[j] : max(start[j], j -
// preceding), following < 0 ? end[j] : min(end[j], j + following)].  preceding < 0: the value is P[hi] of a plain forward
// scan; else following < 0: S[lo] of a plain reverse scan; else P / S are the forward / reverse scans with block = preceding +
// following + 1 and the value is P[hi], S[lo] or combine(S[lo], P[hi]).  Written through out_mode like a scan's result.
struct WinFrameArgs {
    int op;                                 // QE_WSCAN_SUM / MIN / MAX
    int out_mode;                           // QE_WOUT_SUM / MINMAX / AVG / COUNT
    long long n, preceding, following;
    const unsigned int *start, *end;        // first and last row of every row's partition
    const double *p_v, *s_v;                // the scanned pairs (QE_WOUT_ITEM); the pair that is not read may be null
    const unsigned int *p_c, *s_c;
    void *out;
    unsigned long long *out_valid;          // null for COUNT
};
void launch_win_frame(hipStream_t s, const WinFrameArgs &a);
// LAG / LEAD (end null): out[j] = src[j + delta] where that row exists and start[j + delta] == start[j], else zero with
// validity 0.  FIRST_VALUE / LAST_VALUE (end given): out[j] = src[min(max(j + delta, start[j]), end[j])] with that row's validity.
// width 8 / 4, or 0 for a bitmap column; src_valid null = every source row valid; out_valid null = no validity is written
void launch_win_shift(hipStream_t s, int width, const void *src, const uint64_t *src_valid, const uint32_t *start, const uint32_t *end,
                      int64_t n, int64_t delta, void *out, uint64_t *out_valid);

// ---- ordered-set aggregates per group over sorted rows (qe_ordered.hip) ----
// grid cap, in blocks of 256 threads, of the kernels with a lane per group or per run of equal values (262 144 lanes a sweep)
constexpr int kOsaBlocks = 1024;
// The word ranks (`*_prefix`) and the compacted positions (gstart, runpos) below come from bitmap_ranks / bitmap_positions
// (qe_scan.h): prefix[w] = set bits of the words before w, ceil(n / 64) + 1 entries, the last is the total.
// The sorted rows of one (group columns, argument) sort as the per-group kernels read them.  Group g is rows [gstart[g],
// gstart[g + 1]); its argument values are NULL up to first[g] and valid, ascending, from there on.
struct OsaGroups {
    long long n, ngroups;
    const unsigned int *perm;               // source row that stands at sorted position j
    const unsigned int *gstart;             // ngroups + 1 entries, gstart[ngroups] = n
    unsigned int *first;                    // ngroups entries: first valid position of the group (gstart[g + 1]: none)
};
// first[g] by bisection over `valid` (the argument's validity in sorted order; null: every value valid)
void launch_osa_first_valid(hipStream_t s, const OsaGroups &g, const unsigned long long *valid);
// a source-row list per group for gather_column (0xFFFFFFFF: no row).  KEY: the group's first row; DISC: the row of
// v[max(ceil(fraction * c) - 1, 0)], c = valid values; MODE: the row `best` names (launch_osa_mode)
enum { QE_OSA_ROWS_KEY = 0, QE_OSA_ROWS_DISC = 1, QE_OSA_ROWS_MODE = 2 };
void launch_osa_rows(hipStream_t s, const OsaGroups &g, int kind, double fraction, const unsigned long long *best, uint32_t *rows_out);
// PERCENTILE_CONT: out[g] and its validity word (whole words are written); type / data: the SOURCE column (DOUBLE, INT64, INT32)
void launch_osa_percentile_cont(hipStream_t s, const OsaGroups &g, int type, const void *data, double fraction, double *out,
                                unsigned long long *out_valid);
// COUNT_DISTINCT: out[g] = runs of equal values among the group's valid rows = peer bits in [first[g], gstart[g + 1])
void launch_osa_count_distinct(hipStream_t s, const OsaGroups &g, const unsigned long long *peer, const uint32_t *peer_prefix, double *out);
// MODE: best[g] (zeroed by the caller) = max over the group's runs of valid values of (length << 32 | 0xFFFFFFFF - start);
// 0 = no valid value.  runpos: the compacted peer bits, runs + 1 entries, runs = the total that peer_prefix ends with (read
// on the device: the grid is sized by n); pstart / pstart_prefix: the group of a position
void launch_osa_mode(hipStream_t s, const OsaGroups &g, const uint32_t *runpos, const uint32_t *peer_prefix, const unsigned long long *pstart,
                     const uint32_t *pstart_prefix, unsigned long long *best);

// ---- set operations over two concatenated, sorted results (qe_setop.hip) ----
// grid cap, in blocks of 256 threads, of the two bitmap kernels (524 288 rows a sweep)
constexpr int kSetopBlocks = 2048;
// out[i] = table[codes[i]], i < n: the right side's STRING codes into the merged dictionary.  A code outside [0, ncodes) is
// written as 0; nothing is skipped under a NULL
void launch_setop_translate_codes(hipStream_t s, const int *codes, int64_t n, const int *table, int ncodes, int *out);
// bit j of side = perm[j] < nleft: the row at sorted position j comes from the left input.  ceil(n / 64) whole words
void launch_setop_side_bits(hipStream_t s, const uint32_t *perm, int64_t n, int64_t nleft, unsigned long long *side);
// bit j of keep = (j - s) < k for the tuple [s, e) = [gstart[g], gstart[g + 1]) that holds j, g = rank of pstart at j; cL = side
// bits in [s, e), cR = e - s - cL; k = QE_SET_UNION: all ? cL + cR : 1; INTERSECT: all ? min(cL, cR) : (cL && cR); EXCEPT: all ?
// max(cL - cR, 0) : (cL && !cR).  *_prefix: the word ranks of bitmap_ranks (qe_scan.h).  ceil(n / 64) whole words
struct SetopKeepArgs {
    int op, all;                            // QE_SET_*, 0 / 1
    long long n, ntuples;
    const unsigned long long *pstart, *side;
    const unsigned int *pstart_prefix, *side_prefix;
    const unsigned int *gstart;             // ntuples + 1 entries, gstart[ntuples] = n
    unsigned long long *keep;
};
void launch_setop_keep(hipStream_t s, const SetopKeepArgs &a);

// ---- ASOF join over two concatenated, sorted key sets (qe_asof.hip) ----
// grid cap, in blocks of 256 threads, of its three kernels (524 288 rows a sweep)
constexpr int kAsofBlocks = 2048;
// Where the rows of the two sides stand: the concatenation holds `nfirst` rows of one side, then the other side's; right_first:
// the first side is the right one.  perm[j] = row of the concatenation at sorted position j.
struct AsofSides {
    const unsigned int *perm;
    long long n, nfirst;
    int right_first;
};
// bit j of eligible = the row at sorted position j is valid in every key column (validity[k] null: no NULL in that column),
// bit j of right = it is eligible and a right row.  ceil(n / 64) whole words each
struct AsofEligibleArgs {
    AsofSides s;
    int nkeys;
    const unsigned long long *validity[8];  // of the concatenated key columns
    unsigned long long *eligible, *right;
};
void launch_asof_eligible(hipStream_t s, const AsofEligibleArgs &a);
// match[l] = the right row of left row l, or 0xFFFFFFFF, written by the sorted position j that holds l -- every left row once.
// An eligible left row takes k = set bits of `right` below j and the candidate position rpos[k - 1] (backward; none when
// k == 0) or rpos[k] (forward; none when k == the set bits of `right`, which is right_prefix's last entry), and accepts it when pstart has no set bit in (candidate, j] (backward) or
// (j, candidate] (forward): both stand in one partition.  *_prefix: the word ranks of bitmap_ranks (qe_scan.h)
struct AsofPickArgs {
    AsofSides s;
    int forward;
    long long nleft;                        // left rows = entries of match; rpos has room for the n - nleft right rows
    const unsigned long long *eligible, *right, *pstart;
    const unsigned int *right_prefix, *pstart_prefix;
    const unsigned int *rpos;               // ascending positions of the set bits of `right`
    unsigned int *match;
};
void launch_asof_pick(hipStream_t s, const AsofPickArgs &a);
// bit l of matched = match[l] != 0xFFFFFFFF, l < nleft, whole words; identity[l] = l when identity is not null (the rows of
// the LEFT form's own side)
void launch_asof_matched(hipStream_t s, const uint32_t *match, int64_t nleft, unsigned long long *matched, uint32_t *identity);

// ---- range join over two concatenated, sorted key sets (qe_range.hip) ----
// grid cap, in blocks of 256 threads, of its three kernels (524 288 rows a sweep of the two lane-per-row kernels)
constexpr int kRangeBlocks = 2048;
// consecutive output rows that one workgroup of the expansion owns at a time
constexpr int kRangeExpandTile = 2048;
// One sort's ordinals.  The row at sorted position j has k = set bits of `right` below j eligible right rows before it.  A left
// row l writes ord[l] = k, or 0xFFFFFFFF when its bit of `eligible` is 0 -- every left row once.  An eligible right row r
// writes rlist[k] = r (rlist null: not wanted), so rlist becomes the eligible right rows in sorted order; it has room for the
// n - nleft right rows.  eligible / right: the bitmaps of launch_asof_eligible, right_prefix: the word ranks of `right`
struct RangeOrdinalArgs {
    AsofSides s;
    long long nleft;
    const unsigned long long *eligible, *right;
    const unsigned int *right_prefix;
    unsigned int *ord, *rlist;
};
void launch_range_ordinals(hipStream_t s, const RangeOrdinalArgs &a);
// Per left row l < nleft: cnt[l] = ord_hi[l] - ord_lo[l] when both ordinals are there and the difference is positive, else 0;
// emit[l] (emit null: not wanted) = the output rows of l, cnt[l] or (left_join) max(cnt[l], 1); bit l of keep = (cnt[l] != 0) !=
// (anti != 0), whole words, the bits past nleft 0; *longest (zeroed by the caller) = max cnt[l], by an integer atomic max.
// cover (RIGHT / FULL; null otherwise): a zeroed u32 difference array of nright + 1 entries over the positions of rlist; a left
// row with cnt[l] != 0 adds 1 at ord_lo[l] and subtracts 1 at ord_hi[l] (integer atomic adds modulo 2^32)
struct RangeCountArgs {
    long long nleft, nright;
    int left_join, anti;
    const unsigned int *ord_lo, *ord_hi;
    unsigned int *cnt;
    long long *emit;
    unsigned long long *keep;
    unsigned int *longest;
    unsigned int *cover;
};
void launch_range_counts(hipStream_t s, const RangeCountArgs &a);
// RIGHT / FULL: scanned[p] = the exclusive u32 sum of the difference array before p, so list position p < nright is covered by
// scanned[p + 1] left intervals; a covered position sets bit rlist[p] of `matched`, a zeroed bitmap over RIGHT ROWS
struct RangeMarkArgs {
    long long nright;
    const unsigned int *scanned;            // nright + 1 entries
    const unsigned int *rlist;
    unsigned long long *matched;
};
void launch_range_mark(hipStream_t s, const RangeMarkArgs &a);
// The load-balanced expansion: output row o < total belongs to the last emitting left row e with eoff[e] <= o; with l = erow[e]
// (erow null: l = e) and k = o - eoff[e] it writes lrow[o] = l and rrow[o] = cnt[l] ? rlist[ord_lo[l] + k] : 0xFFFFFFFF.  eoff:
// the first output row of each of the nemit emitting left rows, strictly ascending from 0, so a tile of kRangeExpandTile output
// rows meets at most kRangeExpandTile + 1 of them: a workgroup stages those in LDS and every lane searches there
struct RangeExpandArgs {
    long long total, nemit, nleft, nright;
    const long long *eoff;
    const unsigned int *erow;
    const unsigned int *cnt, *ord_lo;       // per left row
    const unsigned int *rlist;              // nright entries
    unsigned int *lrow, *rrow;
};
void launch_range_expand(hipStream_t s, const RangeExpandArgs &a);

// ---- CSV text parsed on the device (qe_csv_device.hip) ----
#pragma GCC visibility push(hidden)   // qe_csv_device.cpp alone calls these
constexpr int kCsvTile = 4096;   // text bytes per wave in the structure passes; the text buffer is zero-padded to whole tiles
// flags word: what the passes found that the host parser would read differently
enum { QE_CSV_QUOTE_RULE = 1, QE_CSV_BAD_NUMBER = 2, QE_CSV_PATCH_OVERFLOW = 4 };
// tile_quotes[t] = the '"' bytes of tile t
void launch_csv_quote_count(hipStream_t s, const unsigned char *text, long long ntiles, long long *tile_quotes);
// The non-empty records of the n text bytes, from the scanned quote counts.  write false: tile_rows[t] = records that start in
// tile t, and QE_CSV_QUOTE_RULE where a '"' is not the enclosing quote of a field; true: rec_start[row] = first byte of the
// record, through the scanned tile_rows
void launch_csv_records(hipStream_t s, bool write, const unsigned char *text, long long n, long long ntiles, const long long *tile_quotes,
                        long long *tile_rows, long long *rec_start, unsigned int *flags);
// The fields of one projected column: row r holds the lenesc[r] >> 1 content bytes from text + begin[r], and lenesc[r] & 1 says
// that they hold "" escapes.  No byte = NULL (empty, "" or missing).
struct CsvFields {
    const unsigned char *text;
    long long nrows;
    long long *begin;
    unsigned int *lenesc;
};
// all: the fields of all ncols columns, column k at k * nrows, written from the record starts
struct CsvSpanArgs {
    CsvFields all;
    long long n;                            // text bytes
    const long long *rec_start;
    const int *field_of;                    // per projected column: field index in the record
    int ncols, max_field;
};
void launch_csv_spans(hipStream_t s, const CsvSpanArgs &a);
// DOUBLE: values (0 under a NULL) and validity; a field that is no number raises QE_CSV_BAD_NUMBER, one that the device
// leaves undecided goes to patch_rows, QE_CSV_PATCH_OVERFLOW past patch_cap.  BOOLEAN: value and validity bitmaps.
// *any_null is raised when a row is NULL
struct CsvConvArgs {
    CsvFields f;
    void *data;
    unsigned long long *validity;
    unsigned int *any_null, *flags;
    long long *patch_rows;
    unsigned int *patch_count, patch_cap;
};
void launch_csv_convert_double(hipStream_t s, const CsvConvArgs &a);
void launch_csv_convert_bool(hipStream_t s, const CsvConvArgs &a);
// data[rows[i]] = values[i], i < n
void launch_csv_scatter_f64(hipStream_t s, double *data, const long long *rows, const double *values, long long n);
// STRING: the dictionary of a column and the codes of its rows, in three steps with a scan between them
struct CsvDictArgs {
    CsvFields f;
    unsigned long long *hash;               // per row: FNV-1a of the unescaped bytes
    unsigned int *slots;                    // open-addressing table of mask + 1 entries (0xFFFFFFFF: free): the row that represents the string
    unsigned int *first;                    // .. the smallest row holding it (0xFFFFFFFF on entry)
    unsigned long long mask;
    unsigned int *row_slot;                 // per row: its entry
    long long *rank;                        // per row: 1 if the row is the first of its string, then (scanned) the code it gives that string
    int *codes;
    long long *dist_row;                    // per code: the first row
    long long *dist_len;                    // per code: unescaped bytes
    unsigned long long *validity;
    unsigned int *any_null;
};
void launch_csv_dict_build(hipStream_t s, const CsvDictArgs &a);   // hash, validity, table, rank (unscanned)
void launch_csv_dict_codes(hipStream_t s, const CsvDictArgs &a);   // rank scanned: codes, dist_row, dist_len
// len[i] = unescaped bytes of field rows[i], i < n
void launch_csv_field_len(hipStream_t s, const CsvFields &f, const long long *rows, long long n, long long *len);
// the unescaped bytes of field rows[i] at packed + off[i], i < n
void launch_csv_pack_fields(hipStream_t s, const CsvFields &f, const long long *rows, long long n, const long long *off, unsigned char *packed);
#pragma GCC visibility pop

// ---- gathers through u32 row ids (qe_kernels.hip): ORDER BY, window, join, per-node ----
// grid caps, in blocks of 256 threads: every caller's, and the join's output columns (with the narrow cap the probe was 0.4 to
// 0.6 % slower than before in every interleaved run, with the wide one it is not: profiles/result_builder_refactor_summary.txt)
constexpr int kGatherBlocks = 8192, kGatherBlocksWide = 16384;
// out[j] = src[rows[j]], or zero for row 0xFFFFFFFF ("no row"); width 4 or 8
void launch_gather_rows(hipStream_t s, int width, const void *src, const uint32_t *rows, int64_t n, void *out, int max_blocks = kGatherBlocks);
// bit j of out = bit rows[j] of src (src null: 1), 0 for row 0xFFFFFFFF; whole words are written
void launch_gather_bits_rows(hipStream_t s, const uint64_t *src, const uint32_t *rows, int64_t n, uint64_t *out, int max_blocks = kGatherBlocks);

// place nbits bits of src at bit offset dst_bit_offset of dst (bitmap words; concatenation of results / gather)
void launch_bitmap_place(hipStream_t s, uint64_t *dst, int64_t dst_bit_offset, const uint64_t *src, int64_t nbits);

}  // namespace qe
