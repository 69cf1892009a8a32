/*
 * ssw_gpu.h -- batch entry points of the MI355X-native Smith-Waterman library.
 *
 * The reference library aligns ONE (query, target) pair per synchronous call
 * (reference src/ssw.h:126-134); its callers loop "for each read: ssw_init; for
 * each target: ssw_align" (reference src/main.c:462-526, src/pyssw.py:120-142,
 * src/ssw_cpp.cpp:319-357).  This header is what such a loop binds instead when
 * it wants GPU throughput: the same parameters, applied to a whole batch of
 * device-resident queries x targets, returning one s_align-equivalent record per
 * pair in the caller's loop order (query-major: reads outer, targets inner).
 * ssw.h's single-pair functions are implemented on top of this path.
 *
 * Plain C ABI: pointers and sizes only.  All functions return 0 on success and a
 * negative value on failure (ssw_gpu_last_error() has the text); there is no CPU
 * fallback -- without a usable gfx950 device every entry point fails.
 */
#ifndef SSW_GPU_H
#define SSW_GPU_H

#include <stddef.h>
#include <stdint.h>
#include "ssw.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ssw_gpu_ctx ssw_gpu_ctx;    /* one device + its streams/workspaces */
typedef struct ssw_gpu_seqs ssw_gpu_seqs;  /* a set of residue-code sequences resident in HBM */

/* Scoring / reporting parameters: the arguments of reference ssw_init + ssw_align
   (src/ssw.h:86, 126-134) that are not the sequences themselves. */
typedef struct {
	const int8_t* mat;   /* n*n scores, mat[target_code*n + read_code] (host pointer) */
	int32_t n;           /* alphabet size, any n >= 1 like the reference: up to 32 letters on the profile kernels; above that (and whenever gapO <= gapE) on the
	                        lane-model kernel -- the reference's answer at CPU-class speed; beyond 128 only the leading 128 x 128 block is addressable by int8 codes */
	uint8_t gapO;        /* weight_gapO */
	uint8_t gapE;        /* weight_gapE */
	uint8_t flag;        /* as ssw_align */
	uint16_t filters;
	int32_t filterd;
	int32_t maskLen;     /* >= 0: used for every query; < 0: readLen/2 per query (reference src/main.c:464) */
	int8_t score_size;   /* as ssw_init: 0, 1 or 2 */
	int8_t mark_mismatch;/* != 0: every returned CIGAR is rewritten on the device the way mark_mismatch() does it (soft clips,
	                        '=' / 'X' runs) and edit_distance receives its return value (reference src/ssw.c:1019-1074) */
} ssw_gpu_params;

/* One alignment: the fields of s_align (reference src/ssw.h:55-66) with the CIGAR
   held in a shared pool instead of a per-result pointer. */
typedef struct {
	uint16_t score1;
	uint16_t score2;
	int32_t ref_begin1;
	int32_t ref_end1;
	int32_t read_begin1;
	int32_t read_end1;
	int32_t ref_end2;
	int32_t cigarLen;    /* 0: no path */
	int32_t edit_distance; /* mark_mismatch()'s return value when params.mark_mismatch is set, else 0 */
	int64_t cigar_off;   /* first word of this CIGAR in the pool returned by ssw_gpu_align_batch */
	uint16_t flag;       /* as s_align.flag */
	uint16_t status;     /* 0 ok; 1 the reference returns NULL here (8-bit overflow with score_size 0) */
} ssw_gpu_result;

/* Per-phase device time of the last batch call, from HIP events on the library's stream. */
typedef struct {
	double total_ms;       /* first launch .. results on host */
	double fill_ms;        /* sum over forward-fill kernel launches */
	int64_t fill_launches; /* (database search: launch groups -- all size classes of one chunk of targets, side by side on several streams) */
	int64_t fill_cells;    /* DP cells actually evaluated by the fill kernel (padding + halo included) */
	int64_t cells;         /* sum of readLen*refLen over the batch (the GCUPS numerator) */
	double reduce_ms;      /* score1/score2/end-position reduction (ssw_gpu_search_topk: the device time of the k_topk selection;
	                          ssw_gpu_align_windows_best / _topk: of the k_groupbest / k_grouptopk selection; ssw_gpu_insert_hist: of k_insertstat) */
	double locate_ms;      /* read_end1 + reverse (begin position) passes */
	double trace_ms;       /* banded traceback + CIGAR re-score */
	int64_t n_word;        /* alignments decided under 16-bit semantics */
	int64_t n_byte;        /* alignments decided under 8-bit semantics */
	/* the fill kernel that evaluated most cells in the call (for roofline accounting) */
	char fill_kernel[48];  /* e.g. "k_fill<10,frame>", "k_chainq<12,frame> x 14 strips", "k_chainq<12,pairs,frame> x 13 strips + 1 of 1", "k_filldb<19,frame>" */
	double fill_ops_per_row; /* VALU instructions of the recurrence per (row, column) of a query pair in that kernel: 6.5 (column frame) / 7.5 / 8.5 / 9;
	                            k_fill8<R> (column frame + blocked row frame, one diagonal add per two rows): its own count per instance, 5.42 at R = 19.
	                            "k_fill8<R,frame> dg" (gaps open from the diagonal candidate only, where the scoring and the target allow it):
	                            max(count, 5.0), the counts being 6/1, 17/3, 28/5, 37/7, 54/11, 63/13 = 4.846, 73/15 = 4.867, 91/19 = 4.789,
	                            101/21 = 4.810 and 111/23 = 4.826 -- the instances from R = 11 on report 5.0; R = 9 and R = 17 have no such form.
	                            The REPORTED value of two instances moved when the adds went in pairs: R = 7 reports 37/7 = 5.286 (was 38/7 = 5.429)
	                            and R = 11 reports 5.0 (was 56/11 = 5.091); every other instance reports what it did.
	                            (With every plain add on its own, as before the adds went in pairs: 38/7, 56/11, 66/13, 76/15, 94/19, 104/21, 114/23.)
	                            k_chainq<R,pairs,..> reports the batch fill's 6.5 / 9 although it merges the two halves' profile entries per row
	                            (one more instruction): a roofline computed from it is understated for that kernel */
	int32_t fill_rows_per_lane;
	int32_t fill_strips;
	int64_t db_repeats;    /* (rounds 1-2: workgroups of the database search that repeated in the int16 form; always 0 since the column-frame form) */
	int64_t fill_pipelined; /* fill launches of the call that ran as a PIPELINED series (main stream / a second stream alternately, two launches in flight, round 6): they overlap,
	                           fill_ms brackets each series as a whole -- fill_ms / fill_launches is then the series' time per launch, not a kernel's duration */
	int64_t win_copied;    /* ssw_gpu_align_windows: target residues copied into temporary sets by the call (0 when every pair took the fast path;
	                          always 0 for the other entry points) */
	int64_t best_flagged;  /* ssw_gpu_align_windows_best: pairs the call handed to the reverse pass and the traceback -- the winners, never more than ngroups
	                          (ssw_gpu_align_windows_topk: the reported slots that pass src/ssw.c:916, never more than ngroups * k);
	                          0 with flag 0 and for the other entry points */
	int64_t db_long_pairs; /* database search (ssw_gpu_align_batch against four or more targets, ssw_gpu_search_db, ssw_gpu_search_topk): the (query, target)
	                          pairs answered by the long class of the database path -- queries above k_filldb's 640 residues on the strip kernel's pair
	                          mode, two targets per job; 0 when there are none and for the other entry points */
	int64_t rescue_windows; /* ssw_gpu_align_windows_mates_rescue: the non-empty rescue slots the call filled; 0 for the other entry points */
	/* new fields are only ever appended here; ssw_gpu_last_timing_sized lets a caller built against an older header keep its layout */
} ssw_gpu_timing;

int ssw_gpu_device_count(void);
ssw_gpu_ctx* ssw_gpu_open(int device);          /* NULL on failure */
void ssw_gpu_close(ssw_gpu_ctx* ctx);
const char* ssw_gpu_last_error(const ssw_gpu_ctx* ctx);   /* ctx may be NULL: error of the last failed open */

/* Upload `count` sequences: codes of sequence i are codes[offsets[i] .. offsets[i+1]). */
ssw_gpu_seqs* ssw_gpu_seqs_upload(ssw_gpu_ctx* ctx, const int8_t* codes, const int64_t* offsets, int32_t count);
/* Same, from ASCII residues: the translation through `table128` (e.g. the reference's nt_table / aa_table,
   src/main.c:72-93, applied per read at src/main.c:476, 504) runs on the device. */
ssw_gpu_seqs* ssw_gpu_seqs_upload_ascii(ssw_gpu_ctx* ctx, const char* text, const int64_t* offsets, int32_t count,
                                        const int8_t* table128);
/* Reverse complement of every sequence of a DNA code set (0..3 -> 3 - code, other codes kept), computed on the device:
   what `ssw_test -r` builds per read on the host (reference src/main.c:95-116, 478-481). */
ssw_gpu_seqs* ssw_gpu_seqs_revcomp(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* s);
/* The sequences of `s` followed by their reverse complements: one set of 2 x count sequences (sequence count + i is the reverse
   complement of sequence i) -- `ssw_test -r` as ONE batch call of 2 N queries (reference src/main.c:478-481, 507-519). */
ssw_gpu_seqs* ssw_gpu_seqs_with_revcomp(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* s);
int ssw_gpu_seqs_download(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* s, int8_t* codes_out);
void ssw_gpu_seqs_free(ssw_gpu_seqs* s);
int32_t ssw_gpu_seqs_count(const ssw_gpu_seqs* s);

/*
 * Align every query to targets [target_first, target_first + target_count).
 * results[q * target_count + t] receives the record of (query q, target target_first + t).
 * cigar_pool (optional) receives a malloc()ed array of *cigar_words BAM-packed words (caller frees).
 *
 * Against four or more short targets the call is ONE database search whatever the flag: scores and end positions of all pairs from a
 * fused kernel; with flag != 0 the pairs that pass the reference's gates (src/ssw.c:916: not when flag == 2 and score1 < filters) go
 * through one batched reverse pass and traceback -- the loop of src/main.c:493-506 without a per-target iteration.  Queries of mixed
 * lengths run side by side.  A call with one query and one target is what ssw_align is made of.
 * Envelope of the database search: gapO > gapE, n <= 32, max(mat) <= 49, targets of at most 65 000 columns.  Queries of 1..640 residues
 * (1..384 where n x 10 x 256 > 65 535, i.e. n >= 26) run on k_filldb; longer ones, up to 65 535 residues, on the strip kernel's pair mode
 * (both halves of a register hold the same query, against two targets of neighbouring length; ssw_gpu_timing.db_long_pairs counts these
 * pairs), as long as one job's scratch -- about 24 bytes per column of the longest target -- fits half of ssw_gpu_get_budget.  Rows
 * outside the envelope are answered exactly by a loop over the targets: one round trip per target.
 */
int ssw_gpu_align_batch(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* queries, const ssw_gpu_seqs* targets,
                        int32_t target_first, int32_t target_count, const ssw_gpu_params* params,
                        ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words);

/*
 * Align an explicit list of (query, target) pairs: results[i] is, bit for bit, the record that
 * ssw_gpu_align_batch(ctx, queries, targets, tidx[i], 1, ...) gives at row qidx[i] -- the loop "for each read: ssw_align
 * against ITS window(s)" of a mapper or variant caller as one call.  Pairs come in any order, repeats allowed.  The CIGAR pool
 * (optional, malloc()ed, caller frees) holds the CIGARs in pair order.  npairs == 0 returns 0 with *cigar_words = 0; an index out of
 * range returns -1 with a message before anything is launched or written.  Every phase stays within ssw_gpu_get_budget(ctx).
 *
 * Fast path (one fused kernel, k_fillpairs: two pairs per 16-lane chain, each half of a register against its own target): gapO > gapE,
 * n <= 32, max(mat) <= 49, queries of 1..640 residues (n x ceil(ceil(len/16)/4) x 256 < 64 KiB), targets of 1..65 000 columns; with
 * flag != 0 the pairs that pass src/ssw.c:916 then go through ONE batched reverse pass and traceback (whatever the size of the target set).
 * Fast path of long reads (the strip kernel's pair mode, k_chainq<R,pairs,form>: two pairs per 64-lane chain, row strips behind a work
 * queue, then k_reduce_pairs): gapO > gapE, n <= 32, queries of 769..65 535 residues, targets of 1..65 000 columns, one job's scratch
 * (about 24 bytes per target column) within half of ssw_gpu_get_budget; no limit on max(mat) -- the form of the recurrence follows the
 * scores.  Same records, same flagged phases, pairs of both envelopes in one call in any order.
 * Queries of 641..768 residues are on NEITHER fast path (k_fillpairs ends at 40 rows per lane, the strip kernel's pair mode starts where
 * every query has at least two strips).  They and every other pair -- empty sequences, gapO <= gapE, wider alphabets, larger scores of
 * short reads, targets over 65 000 columns -- are answered exactly but SLOWLY: one internal ssw_gpu_align_batch per distinct target over
 * the subset of its queries (gathered on the device).
 */
int ssw_gpu_align_pairs(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* queries, const ssw_gpu_seqs* targets,
                        const int32_t* qidx, const int32_t* tidx, int64_t npairs,
                        const ssw_gpu_params* params, ssw_gpu_result* results,
                        uint32_t** cigar_pool, int64_t* cigar_words);

/*
 * Align a list of (query, WINDOW of a resident target) pairs: results[i] is, bit for bit, the record ssw_gpu_align_pairs gives for query
 * qidx[i] against a target that consists of residues [tbeg[i], tbeg[i] + tlen[i]) of target tidx[i] uploaded as a sequence of its own -- and
 * through it the reference's ssw_init + ssw_align(profile, ref + tbeg, tlen, ...) answer.  The loop of a mapper, variant caller or
 * assembler whose reference genome stays on the device while every batch of reads brings a fresh list of (read, chromosome, position,
 * length) candidates: the host uploads 16 bytes per pair and nothing else about the targets.  All positions (ref_begin1, ref_end1, ref_end2)
 * are WINDOW-RELATIVE (add tbeg[i] for target coordinates); -1 sentinels stay -1.  The CIGAR pool (optional, malloc()ed, caller frees) holds
 * the CIGARs in pair order, as for ssw_gpu_align_pairs.
 * Pairs in any order; repeats, overlapping windows, identical windows and windows of different targets are all allowed.  tlen[i] == 0 gives
 * the record of an empty target.  npairs == 0 returns 0 with *cigar_words = 0.  qidx / tidx out of range, tbeg[i] < 0, tlen[i] < 0 or
 * tbeg[i] + tlen[i] beyond the end of target tidx[i] return -1 with a message that names the pair, before anything is launched or written:
 * nothing is clamped, a window that leaves its chromosome is a caller's bug.  SSW_GPU_BUSY, the context lock and ssw_gpu_last_timing behave
 * as for ssw_gpu_align_pairs; every phase stays within ssw_gpu_get_budget(ctx) (the window table, 32 bytes per pair, is an input of the call
 * like the job list, not scratch).
 *
 * Fast path: ssw_gpu_align_pairs' two envelopes with "target" read as "window" -- gapO > gapE, n <= 32, windows of 1..65 000 columns and
 * either queries of 1..640 residues with max(mat) <= 49 (k_fillpairs) or queries of 769..65 535 residues (the strip kernel's pair mode,
 * any max(mat), a job's scratch within half the budget) --, for EVERY flag and whatever the size of the resident target set (2^31 residues
 * and more).  On that path no target residue is copied: the fill, the reverse pass, the traceback and mark_mismatch read the window where it
 * lies, through a per-pair (64-bit start, length) table built on the device.  Everything else -- queries of 641..768 residues, longer
 * windows, empty ones, gapO <= gapE, wider alphabets, larger scores of short reads -- is answered exactly and may be slow: those windows
 * are gathered on the device into temporary sets (identical windows once) and handed to ssw_gpu_align_pairs' path;
 * ssw_gpu_timing.win_copied counts their residues.
 * Several devices, or several workers on one: ssw_gpu_pool_align_windows.
 * Not provided (yet): a CLI option, a strand flag per pair (both strands: ssw_gpu_seqs_with_revcomp on the
 * reads and qidx = count + i), a wider envelope (queries of 641..768 residues, windows over 65 000 columns on the fast path).
 */
int ssw_gpu_align_windows(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* queries, const ssw_gpu_seqs* targets,
                          const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                          int64_t npairs, const ssw_gpu_params* params, ssw_gpu_result* results,
                          uint32_t** cigar_pool, int64_t* cigar_words);

/*
 * Best candidate window per read: ssw_gpu_align_windows over candidates in GROUPS, kept to the best candidate of every group -- what a
 * mapper with a resident genome does with the candidate windows of a read (one per surviving seed chain, usually on both strands): which
 * one is best, how close the runner-up is (the input of a mapping quality), and begin positions + CIGAR of the winner alone.
 * Group g is candidates [cand_off[g], cand_off[g + 1]) of the four per-candidate arrays (cand_off[0] == 0, cand_off[ngroups] = the number of
 * candidates); candidate i means exactly what pair i of ssw_gpu_align_windows means.  qidx is per candidate: a read's forward and
 * reverse-complement candidates share a group (ssw_gpu_seqs_with_revcomp on the reads, qidx = count + i for the reverse strand).
 * A candidate is ELIGIBLE when its ssw_gpu_align_windows record has status 0, score1 > 0 and score1 >= min_score (ssw_gpu_search_topk's rule).
 * Ranking: score1 descending, then position in the group ascending; two identical windows in one group are two candidates.
 *   sel[g]      best / second: positions (relative to cand_off[g]) of the first two of that order, -1 where there is none; n_eligible;
 *               second_score1.  These do not depend on params->flag.
 *   results[g]  bit for bit the record ssw_gpu_align_windows gives for the single pair `best` with the caller's flag, filters, filterd,
 *               maskLen, score_size and mark_mismatch (window-relative positions); a group without an eligible candidate -- an empty group
 *               too -- gets ssw_gpu_search_topk's padding record (zeros, ref_begin1 = read_begin1 = -1, cigar_off = -1);
 *   cigar_pool  (optional, malloc()ed, caller frees) the winners' CIGARs in group order.
 * The forward fill runs once over all candidates (k_fillpairs and, for reads of 769 residues and more, the strip kernel's pair mode, as for
 * ssw_gpu_align_windows: no target residue is copied inside the two envelopes); the selection runs on the device (k_groupbest); one record per GROUP comes to the host; the reverse pass, the traceback and
 * mark_mismatch run over the winners only (ssw_gpu_timing.best_flagged), their fill records reused.
 * Candidates outside the fast-path envelopes (empty ones, reads of 641..768 residues, windows over 65 000 columns, gapO <= gapE, alphabets
 * over 32 letters, max(mat) > 49 with reads up to 640 residues) are exact in any mix, inside one group too: they take ssw_gpu_align_windows' fallback at flag 0 first, their
 * records are uploaded beside the fill's, the DEVICE selects over everything, and those of them that win take the fallback once more
 * with the caller's flag.
 * Memory: the state that outlives a fill launch -- 48 bytes of record and 4 bytes of slot map per candidate, 64 bytes of output (record +
 * selection) and 8 of offsets per group -- is an input / output of the call like the window table, not scratch under ssw_gpu_get_budget: 52 bytes per
 * candidate (within the 64 this entry point allows itself) beyond what ssw_gpu_align_windows needs.  Fill launches are cut to the budget
 * as there.
 * Errors (-1 with a message that names the group or the pair, before anything is launched or written): a NULL array, cand_off[0] != 0, a
 * decreasing cand_off, more than 0x7fffff00 candidates, an index or window out of range (ssw_gpu_align_windows' text), sequences of
 * another context.  ngroups == 0 returns 0 with *cigar_words = 0.  SSW_GPU_BUSY and the context lock as for ssw_gpu_align_windows.
 * ssw_gpu_last_timing: reduce_ms is the device time of k_groupbest; best_flagged the winners handed to the reverse pass / traceback.
 * Not provided (yet): a CLI option, building the survivor list of the
 * flagged stage on the device (the winners' records make one round trip to the host), a fast path for reads of 641..768 residues.
 * More than the best two per group: ssw_gpu_align_windows_topk.  Several devices: ssw_gpu_pool_align_windows_topk with k = 2 (no pool
 * variant of this entry point: see there).
 */
typedef struct {
	int32_t best;          /* position in the candidate list of the group's best eligible candidate; -1: none */
	int32_t second;        /* the runner-up under the same ranking; -1: fewer than two eligible */
	int32_t n_eligible;    /* eligible candidates of the group */
	uint16_t second_score1;/* score1 of `second` (0 when second == -1) */
	uint16_t pad;          /* 0 */
} ssw_gpu_best;
int ssw_gpu_align_windows_best(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* queries, const ssw_gpu_seqs* targets,
                               const int64_t* cand_off, int64_t ngroups,
                               const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                               const ssw_gpu_params* params, int32_t min_score,
                               ssw_gpu_best* sel, ssw_gpu_result* results,
                               uint32_t** cigar_pool, int64_t* cigar_words);

/*
 * Best k candidate windows per read: ssw_gpu_align_windows_best with k ranks per group -- the primary alignment of a read AND its
 * secondaries (the other loci of a repeat, the alternate haplotype, the second strand) with begin positions and CIGARs, and the number of
 * near-best hits a mapping quality is computed from, in one call and one forward fill.
 * Groups, candidates, eligibility (status 0, score1 > 0, score1 >= min_score) and ranking (score1 descending, then position in the group
 * ascending; identical windows are distinct candidates) are exactly ssw_gpu_align_windows_best's.  1 <= k <= SSW_GPU_GROUP_TOPK_MAX.
 *   pos[g * k + r]      position, relative to cand_off[g], of the r-th ranked eligible candidate of group g; -1 past the last.  Rank r >= 1 is
 *                       reported only if its score1 >= score1(rank 0) - max_drop (max_drop < 0: no cut; 0: ties with the best only); the
 *                       order is descending, so the cut truncates the list: every slot after the first -1 is -1.
 *   n_eligible[g]       eligible candidates of the group, whatever k and max_drop are (as ssw_gpu_best.n_eligible).
 *   results[g * k + r]  bit for bit the record ssw_gpu_align_windows gives for that single pair with the caller's flag, filters, filterd,
 *                       maskLen, score_size and mark_mismatch (window-relative positions); slots with pos == -1 hold ssw_gpu_search_topk's
 *                       padding record (zeros, ref_begin1 = read_begin1 = -1, cigar_off = -1).
 *   cigar_pool          (optional, malloc()ed, caller frees) the CIGARs in (g, r) order.
 * pos and n_eligible do not depend on params->flag.  With k = 1, pos / results / the pool equal sel.best / results / the pool of
 * ssw_gpu_align_windows_best; with k = 2 and max_drop < 0, pos[2 g + 1] == sel[g].second and results[2 g + 1].score1 == sel[g].second_score1.
 * The forward fill runs once over all candidates as for ssw_gpu_align_windows_best; the selection runs on the device (k_grouptopk: one
 * 16-lane row per group, rank by rank); k records per group come to the host; ONE survivor list of all reported slots goes through the
 * reverse pass, the traceback and mark_mismatch, the fill records reused.  Candidates outside the fast-path envelopes are treated as
 * there: the fallback at flag 0 first, the device ranks everything, those that place take the fallback once more with the caller's flag.
 * Memory (inputs / outputs of the call like the window table, not scratch under ssw_gpu_get_budget): per candidate 48 bytes of record and
 * 4 of slot map, per group 52 k + 4 bytes of output (k records, k positions, one count) and 8 of offsets.
 * Errors (-1 with a message, before anything is launched or written): k outside 1..SSW_GPU_GROUP_TOPK_MAX, a NULL array, cand_off[0] != 0,
 * a decreasing cand_off, more than 0x7fffff00 candidates, ngroups * k beyond 0x7fffff00, an index or window out of range
 * (ssw_gpu_align_windows' text), sequences of another context.  ngroups == 0 returns 0 with *cigar_words = 0.  SSW_GPU_BUSY and the
 * context lock as for ssw_gpu_align_windows.
 * ssw_gpu_last_timing: reduce_ms is the device time of k_grouptopk; best_flagged the reported slots that pass src/ssw.c:916 (all of them
 * unless flag == 2 and score1 < filters) -- the pairs handed to the reverse pass / traceback, never more than ngroups * k, 0 at flag 0.
 * Several devices, or several workers on one: ssw_gpu_pool_align_windows_topk.
 * Not provided (yet): a CLI option, a strand flag per pair, building the survivor list on the device.
 */
#define SSW_GPU_GROUP_TOPK_MAX 64
int ssw_gpu_align_windows_topk(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* queries, const ssw_gpu_seqs* targets,
                               const int64_t* cand_off, int64_t ngroups,
                               const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                               const ssw_gpu_params* params, int32_t k, int32_t min_score, int32_t max_drop,
                               int32_t* pos, int32_t* n_eligible, ssw_gpu_result* results,
                               uint32_t** cigar_pool, int64_t* cigar_words);

/*
 * Best candidate pair per read pair: the step of a paired-end mapper between seeding and SAM output.  A fragment has two mates, each with
 * its own candidate windows; wanted is not the best window of either mate but the best COMBINATION -- one candidate of mate 1 and one of
 * mate 2 on the same target, on opposite strands, a plausible insert apart -- and how far the next-best combination is.
 * cand_off has 2 * nfrag + 1 offsets: group 2 f holds the candidates of mate 1 of fragment f, group 2 f + 1 those of mate 2.  Candidates,
 * their four arrays and eligibility (status 0, score1 > 0, score1 >= min_score) are exactly ssw_gpu_align_windows_best's; a group holds at
 * most SSW_GPU_MATES_GROUP_MAX candidates.  Candidate i is on the minus strand iff qidx[i] >= nfwd (ssw_gpu_seqs_with_revcomp's
 * convention: nfwd = the number of forward reads; nfwd = queries->count: everything on the plus strand).
 * Per eligible candidate i, from its flag-0 record `rec`, in 64-bit arithmetic and target coordinates:
 *   E = tbeg[i] + rec.ref_end1          the last column of the alignment;
 *   B = E - len(query qidx[i]) + 1      the ESTIMATED first column, signed and never clamped (a read hanging over column 0 has B < 0).
 * B is an estimate by design -- begin positions do not exist before the reverse pass, which runs over the winners only; an alignment
 * with gaps or clipping begins elsewhere.  It decides which combinations count as proper, nothing else: the caller computes TLEN from the
 * winners' real ref_begin1 / ref_end1.
 * A combination (a of mate 1, b of mate 2) is PROPER (FR library) iff tidx[a] == tidx[b], the strands differ, and, with p the plus-strand
 * and m the minus-strand one, min_insert <= E(m) - B(p) + 1 <= max_insert.  Its score is
 *   S(a, b) = score1(a) + score1(b) - (proper ? 0 : unpaired_penalty)            (signed)
 * Ranking over eligible x eligible: S descending, then position of a, then position of b ascending -- one total order; a proper and an
 * improper combination of equal S tie-break by position only.
 *   sel[f]          pos1 / pos2: the first combination of that order, positions relative to the groups' cand_off; score: its S;
 *                   second_score: S of the second combination (0 when there is none: n_eligible1 * n_eligible2 < 2); n_proper: proper
 *                   combinations among eligible x eligible; proper: whether the chosen one is.  When only ONE mate has an eligible
 *                   candidate it is chosen by ssw_gpu_align_windows_best's rule (score1 descending, position ascending): the other pos is
 *                   -1, score its score1, second_score the group's runner-up score1, proper = n_proper = 0.  Neither: both -1, the rest 0.
 *                   sel does not depend on params->flag.  With unpaired_penalty == 0, pos1 / pos2 equal ssw_gpu_align_windows_best's
 *                   `best` of groups 2 f and 2 f + 1.
 *   results[2 f + h]  bit for bit the record ssw_gpu_align_windows gives for the chosen candidate of mate h + 1 with the caller's flag,
 *                   filters, filterd, maskLen, score_size and mark_mismatch (window-relative positions); the padding record (zeros,
 *                   ref_begin1 = read_begin1 = -1, cigar_off = -1) where pos is -1;
 *   cigar_pool      (optional, malloc()ed, caller frees) the winners' CIGARs in (fragment, mate) order.
 * The forward fill runs once over all candidates as for ssw_gpu_align_windows_best; the selection runs on the device (k_matebest: one
 * 16-lane row per fragment); 32 bytes of selection and two records per fragment come to the host; the reverse pass, the traceback and
 * mark_mismatch run over the winners only, their fill records reused.  Candidates outside the fast-path envelopes are exact in any mix,
 * inside one fragment too, by ssw_gpu_align_windows_best's route: the fallback at flag 0 first, their records uploaded beside the fill's,
 * the fallback once more for those that win.
 * Memory (inputs / outputs of the call like the window table, not scratch under ssw_gpu_get_budget): per candidate 48 bytes of record, 4
 * of slot map and a side table of 16 (tbeg, tidx, read length | strand); per fragment 128 bytes of output (two records, one selection)
 * and 16 of offsets; under a pair model (ssw_gpu_align_windows_mates_model) 2 bytes per entry of the penalty table.  Fill launches are
 * cut to the budget as for ssw_gpu_align_windows.
 * Errors (-1 with a message that names the fragment or the pair, before anything is launched or written): a NULL array, cand_off[0] != 0,
 * a decreasing cand_off, a group of more than SSW_GPU_MATES_GROUP_MAX candidates (pos1 * n2 + pos2 has to fit the 32-bit half of a
 * selection key with room to spare), 2 * nfrag or the candidate count beyond 0x7fffff00, nfwd outside [0, queries->count], min_insert < 0
 * or min_insert > max_insert, unpaired_penalty outside 0 .. 65535, an orientation outside 0 .. 2, an index or window out of range (ssw_gpu_align_windows' text),
 * sequences of another context.  nfrag == 0 returns 0 with *cigar_words = 0.  SSW_GPU_BUSY and the context lock as for
 * ssw_gpu_align_windows.
 * ssw_gpu_last_timing: reduce_ms is the device time of k_matebest; best_flagged the winners handed to the reverse pass / traceback (at
 * most 2 * nfrag; 0 at flag 0).
 * Library orientation (ssw_gpu_align_windows_mates_lib; ssw_gpu_align_windows_mates is that call with SSW_GPU_MATES_FR): which strands
 * and which order make a combination of a (mate 1) and b (mate 2) on one target proper.  D is the span that has to lie in
 * min_insert .. max_insert:
 *   SSW_GPU_MATES_FR   strands differ; p the plus-strand, m the minus-strand candidate:  D = E(m) - B(p) + 1   (reads point at each other)
 *   SSW_GPU_MATES_RF   strands differ;                                                    D = E(p) - B(m) + 1   (the minus-strand mate upstream)
 *   SSW_GPU_MATES_FF   strands equal;  both plus:  D = E(b) - B(a) + 1 (mate 1 upstream);  both minus:  D = E(a) - B(b) + 1 (mate 2 upstream)
 * Nothing else depends on it: S, the ranking, n_proper's meaning, the one-mate case, the records and the CIGAR order.  In k_matebest it
 * is one wave-uniform argument.  An orientation outside 0 .. 2 returns -1 with a message before anything is launched or written.
 * Over several contexts or devices: ssw_gpu_pool_align_windows_mates below.  C++: BatchAligner::AlignWindowsMates (ssw_gpu_cpp.h).
 * Mate rescue -- aligning a mate without a usable candidate where the other mate's anchors and the insert range put it:
 * ssw_gpu_align_windows_mates_rescue below.
 * An insert-size penalty per span in place of the flat "every proper combination costs the same": ssw_gpu_align_windows_mates_model below.
 * Estimating min_insert / max_insert, the orientation and the model's table from a first batch of reads: ssw_gpu_insert_hist and
 * ssw_gpu_insert_fit below.
 * Not provided: more than the best two combinations; MAPQ; a CLI option.
 */
#define SSW_GPU_MATES_GROUP_MAX 4096
#define SSW_GPU_MATES_FR 0
#define SSW_GPU_MATES_RF 1
#define SSW_GPU_MATES_FF 2
typedef struct {
	int32_t pos1, pos2;          /* chosen candidate of mate 1 / mate 2, relative to its group's cand_off; -1: none */
	int32_t n_eligible1, n_eligible2;
	int32_t score;               /* pair score S of the chosen combination; with one mate only: its score1; 0: nothing chosen */
	int32_t second_score;        /* S of the second combination in the ranking (one mate only: second best score1 of that group); 0 when there is none */
	int32_t n_proper;            /* proper combinations among eligible x eligible */
	uint16_t proper;             /* 1: the chosen combination is proper */
	uint16_t pad;                /* 0 */
} ssw_gpu_mates;                 /* 32 bytes */
int ssw_gpu_align_windows_mates(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* queries, const ssw_gpu_seqs* targets,
                                const int64_t* cand_off, int64_t nfrag,
                                const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                                int32_t nfwd,
                                const ssw_gpu_params* params, int32_t min_score,
                                int32_t min_insert, int32_t max_insert, int32_t unpaired_penalty,
                                ssw_gpu_mates* sel, ssw_gpu_result* results,
                                uint32_t** cigar_pool, int64_t* cigar_words);
int ssw_gpu_align_windows_mates_lib(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* queries, const ssw_gpu_seqs* targets,
                                    const int64_t* cand_off, int64_t nfrag,
                                    const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                                    int32_t nfwd,
                                    const ssw_gpu_params* params, int32_t min_score,
                                    int32_t min_insert, int32_t max_insert, int32_t unpaired_penalty, int32_t orientation,
                                    ssw_gpu_mates* sel, ssw_gpu_result* results,
                                    uint32_t** cigar_pool, int64_t* cigar_words);

/*
 * Mate rescue on the device: ssw_gpu_align_windows_mates_lib with the missing mate looked for where its partner says it must be.  Seeding
 * misses a diverged, repetitive or short mate; its fragment then has no proper combination although the other mate is well anchored.
 * Here every group gets max_anchors RESCUE SLOTS behind the caller's candidates, filled on the device between the forward fill of the
 * caller's candidates and the selection; only non-empty slots cost any fill.  All arguments before mate_q, and params .. orientation,
 * mean what they mean for ssw_gpu_align_windows_mates_lib; E, B, eligibility and the proper test are the ones defined there.
 * With A = max_anchors, P = rescue_pad, L = the length of read mate_q[2 f + h], mn / mx = min_insert / max_insert:
 *   Anchors of mate h of fragment f: the caller's candidates of the OTHER mate that are eligible (status 0, score1 > 0, score1 >=
 *     min_score) and have score1 >= anchor_min_score, ranked by score1 descending, then position ascending; anchor r = 0 .. A - 1 is the
 *     r-th of that order.
 *   Rescue slot r of mate h is EMPTY (tbeg 0, tlen 0) when there is no r-th anchor, or when the anchor already has a proper partner
 *     among the caller's eligible candidates of mate h.  Otherwise it lies on the anchor's target, on the strand a proper partner needs
 *     (FR, RF: the opposite of the anchor's; FF: the same), with query mate_q[2 f + h] on the plus and nfwd + mate_q[2 f + h] on the minus
 *     strand, and its window is the set of columns a proper partner can occupy (the orientation table above says which of the two lies
 *     downstream), both ends inclusive:
 *       rescued mate downstream:  [B(anchor) + mn - L - P,  B(anchor) + mx - 1 + P]
 *       rescued mate upstream:    [E(anchor) + 1 - mx - P,  E(anchor) - mn + L + P]
 *     clipped to [0, len(target) - 1]; fewer than one column left: the slot is empty.  (A window is cut at 2^31 - 1 columns.)
 *     Rescue windows are never generated from rescue candidates.
 *   The AUGMENTED list: group 2 f + h = the caller's candidates in their order, then the A slots.  sel, results, *cigar_pool and
 *     *cigar_words equal, bit for bit, what ssw_gpu_align_windows_mates_lib returns for that list with the same remaining arguments:
 *     pos1 / pos2 are positions in the augmented group (a value >= the caller's group size names slot pos - size), n_eligible* and
 *     n_proper count the augmented list; an empty slot is the record of an empty target -- score 0, never eligible.
 *   origin[2 f + h]: window and query of the chosen candidate of mate h + 1, anchor as in the struct; where pos is -1: tbeg 0, tlen 0,
 *     tidx -1, qidx -1, anchor -1.  Positions of results are window-relative: add origin.tbeg (the winner's window may not be the caller's).
 * On the device: k_materescue (k_matebest's geometry and digests: one 16-lane row per fragment) reads the anchors' records where the fill
 * left them and writes 24 bytes per slot; the slot table comes to the host; the non-empty slots are planned and filled like any other
 * candidates (k_fillpairs / the strip kernel's pair mode; outside the envelopes the fallback at flag 0 first, and once more with the
 * caller's flag where they win), their records appended to the same device array; k_matebest runs over the augmented list; the
 * winners-only reverse pass and traceback are unchanged.
 * Memory beyond ssw_gpu_align_windows_mates_lib's (inputs / outputs of the call, not scratch under ssw_gpu_get_budget): 24 bytes per slot
 * (2 * nfrag * A slots), the record (48), slot map (4), side table (16) and window table (32) entries of the slots, and 8 bytes of mate_q
 * per fragment; on the host the augmented copy of the four candidate arrays (20 bytes per candidate and slot).  Under a pair model
 * (ssw_gpu_align_windows_mates_rescue_model) the penalty table's device copy, 2 bytes per entry, uploaded once per call.
 * Errors (-1 with a message that names the fragment, mate or pair, before anything is launched or written): every check of
 * ssw_gpu_align_windows_mates_lib; queries->count != 2 * nfwd (the reverse complements must be resident: ssw_gpu_seqs_with_revcomp);
 * mate_q or origin NULL; a mate_q outside [0, nfwd); a caller's candidate of group g whose qidx is neither mate_q[g] nor nfwd + mate_q[g];
 * max_anchors outside 1 .. SSW_GPU_RESCUE_ANCHORS_MAX; rescue_pad outside 0 .. 65535; anchor_min_score < 0; a group whose size plus
 * max_anchors exceeds SSW_GPU_MATES_GROUP_MAX.  nfrag == 0 returns 0 with *cigar_words = 0.  SSW_GPU_BUSY and the context lock as for
 * ssw_gpu_align_windows.
 * ssw_gpu_last_timing: rescue_windows is the number of non-empty slots; reduce_ms the device time of k_materescue plus k_matebest;
 * fill_ms, fill_launches and fill_cells cover both fills.  The augmented copy and the slot table are host work per candidate and slot
 * whether or not a window is filled (measured: DESIGN 6.18): a list with nothing to rescue is cheaper through
 * ssw_gpu_align_windows_mates_lib.
 * Under a pair model (an insert-size penalty per span): ssw_gpu_align_windows_mates_rescue_model below.
 * Not provided: a pool variant and a BatchAligner method; a CLI option; rescue from rescue candidates.
 */
#define SSW_GPU_RESCUE_ANCHORS_MAX 8
typedef struct {            /* where the chosen candidate of a mate came from: 24 bytes */
	int64_t tbeg;           /* its window, target coordinates */
	int32_t tlen;
	int32_t tidx;
	int32_t qidx;           /* the query it was aligned with (strand included) */
	int32_t anchor;         /* -1: one of the caller's candidates; >= 0: a rescue window, generated from the candidate at this position of the
	                           OTHER mate's group */
} ssw_gpu_rescued;
int ssw_gpu_align_windows_mates_rescue(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* queries, const ssw_gpu_seqs* targets,
                                       const int64_t* cand_off, int64_t nfrag,
                                       const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                                       int32_t nfwd,
                                       const int32_t* mate_q,      /* [2 nfrag]: forward read index, in [0, nfwd), of mate h of fragment f at 2 f + h */
                                       const ssw_gpu_params* params, int32_t min_score,
                                       int32_t min_insert, int32_t max_insert, int32_t unpaired_penalty, int32_t orientation,
                                       int32_t max_anchors, int32_t anchor_min_score, int32_t rescue_pad,
                                       ssw_gpu_mates* sel, ssw_gpu_result* results, ssw_gpu_rescued* origin,
                                       uint32_t** cigar_pool, int64_t* cigar_words);

/*
 * Pair model: ssw_gpu_align_windows_mates_lib's four pairing arguments plus an optional INSERT-SIZE PENALTY TABLE, so that a proper
 * combination is priced by where its span D lies in the library's insert distribution, as a paired-end mapper scores it, and not merely
 * by D being inside min_insert .. max_insert.  Groups, candidates and eligibility, E and B, the orientation table that defines D, the
 * meaning of proper (one target, the orientation's strands, min_insert <= D <= max_insert), n_proper and proper, the one-mate case, the
 * ranking order (S descending, then pos1, then pos2 ascending), the records and the CIGAR order are exactly
 * ssw_gpu_align_windows_mates_lib's.  Only the score of a combination changes:
 *   S(a, b) = score1(a) + score1(b) - (proper ? insert_penalty[D - min_insert] : unpaired_penalty)            (signed)
 * insert_penalty is a host array of max_insert - min_insert + 1 entries, entry i for span D = min_insert + i, read during the call only;
 * NULL stands for all zero.  The table is used AS GIVEN: it is not clamped against unpaired_penalty, so an entry above unpaired_penalty
 * ranks that proper combination below an improper one of equal score sum (proper / n_proper still report properness as defined above).
 * A caller who wants "a proper pair never scores below an improper one" caps the table at unpaired_penalty.  Entries are 0 .. 65535 like
 * unpaired_penalty, so S >= 1 + 1 - 65535 = -65533 as before; second_score == 0 still means "no second combination" only when
 * n_eligible1 * n_eligible2 < 2 (a real S of 0 is possible under any penalty, as with the flat rule).
 * With insert_penalty == NULL or an all-zero table, sel, results, cigar_off and the pool words are bit for bit
 * ssw_gpu_align_windows_mates_lib's.  A table for a normal insert distribution on BWA-MEM's scale: ssw_amd.insert_penalty_normal
 * (Python; plain host arithmetic).
 * ssw_gpu_align_windows_mates_model           ssw_gpu_align_windows_mates_lib under the model.
 * ssw_gpu_align_windows_mates_rescue_model    ssw_gpu_align_windows_mates_rescue under the model: the rescue rule -- anchors, the "already has
 *     a proper partner" test, the window formulas, clipping -- does not look at the table, so the slot table is the flat call's; only the
 *     final selection over the augmented list does, and its answer is bit for bit ssw_gpu_align_windows_mates_model's over that list.
 * ssw_gpu_pool_align_windows_mates_model (further down)   ssw_gpu_pool_align_windows_mates under the model.
 * On the device: k_matebest's combination loop already computes D for the proper test; with a table it subtracts one 16-bit global load
 * at D - min_insert where the flat rule subtracts nothing (no LDS: the selection's 18 KiB per workgroup stay as they are).
 * Memory beyond the sibling's (an input of the call, not scratch under ssw_gpu_get_budget): the device copy of the table, 2 bytes per
 * entry (at most 128 KiB), uploaded once per call on the call's stream -- also when the rescue stage runs.
 * Errors (-1 with a message, before anything is launched or written): model == NULL; a non-NULL table with max_insert - min_insert + 1 >
 * SSW_GPU_INSERT_TABLE_MAX (with a NULL table the range stays unlimited); every refusal of the sibling, applied to the model's fields.
 * C++: BatchAligner::AlignWindowsMates' insert_penalty argument.  Python: the insert_penalty keyword of Context.align_windows_mates,
 * Context.align_windows_mates_rescue and Pool.align_windows_mates.
 * The distribution itself, estimated from data: ssw_gpu_insert_hist and ssw_gpu_insert_fit below.
 * Not provided: MAPQ; a pool or BatchAligner variant of the rescue call; a CLI option.
 */
#define SSW_GPU_INSERT_TABLE_MAX 65536
typedef struct {
	int32_t min_insert, max_insert;      /* as ssw_gpu_align_windows_mates_lib */
	int32_t unpaired_penalty;            /* 0 .. 65535 */
	int32_t orientation;                 /* SSW_GPU_MATES_FR / _RF / _FF */
	const uint16_t* insert_penalty;      /* host pointer: max_insert - min_insert + 1 entries, entry i for span D = min_insert + i; NULL: all zero */
} ssw_gpu_pair_model;
int ssw_gpu_align_windows_mates_model(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* queries, const ssw_gpu_seqs* targets,
                                      const int64_t* cand_off, int64_t nfrag,
                                      const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                                      int32_t nfwd,
                                      const ssw_gpu_params* params, int32_t min_score,
                                      const ssw_gpu_pair_model* model,
                                      ssw_gpu_mates* sel, ssw_gpu_result* results,
                                      uint32_t** cigar_pool, int64_t* cigar_words);
int ssw_gpu_align_windows_mates_rescue_model(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* queries, const ssw_gpu_seqs* targets,
                                             const int64_t* cand_off, int64_t nfrag,
                                             const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                                             int32_t nfwd,
                                             const int32_t* mate_q,
                                             const ssw_gpu_params* params, int32_t min_score,
                                             const ssw_gpu_pair_model* model,
                                             int32_t max_anchors, int32_t anchor_min_score, int32_t rescue_pad,
                                             ssw_gpu_mates* sel, ssw_gpu_result* results, ssw_gpu_rescued* origin,
                                             uint32_t** cigar_pool, int64_t* cigar_words);

/*
 * Insert sizes of a library, estimated from data: the numbers every mates call above takes from its caller -- min_insert, max_insert, the
 * orientation, the pair model's table -- bootstrapped from a first batch of reads, as BWA-MEM's mem_pestat does.  The spans are measured
 * with THIS library's definition, the D that k_matebest tests and indexes the penalty table with (E from the flag-0 fill, B = E - len + 1
 * an estimate), not with a mapper's TLEN from real begin positions: where reads are clipped or gapped the two differ, and a table built
 * from one would be shifted against the D it is later indexed with.
 * ssw_gpu_insert_hist: groups, candidates, nfwd and strand, eligibility, E and B mean what they mean for ssw_gpu_align_windows_mates_lib.
 * Per fragment f:
 *   1. a and b are the candidates ssw_gpu_align_windows_best would return as `best` of groups 2 f and 2 f + 1 (score1 descending, then
 *      position ascending, over eligible candidates only).  Either group has none: the fragment stops here.  Otherwise n_both++.
 *   2. With that call's second_score1 of either group (0 with fewer than two eligible candidates; an ineligible runner-up never counts):
 *      score1(best) - second_score1 < min_margin for either mate stops the fragment.  Otherwise n_unique++.  min_margin == 0 admits ties,
 *      and the first by position is the best.
 *   3. tidx[a] != tidx[b] stops the fragment.  Otherwise n_same++.
 *   4. For each orientation o of SSW_GPU_MATES_FR, _RF, _FF independently: when the strands of a and b satisfy o's strand rule (they
 *      differ for FR and RF, are equal for FF), D_o is computed by the orientation table above, in 64-bit and never clamped;
 *      0 <= D_o <= max_span: hist[o][D_o]++ and n_in[o]++; otherwise n_out[o]++.
 * A fragment with differing strands is tested under FR and under RF.  The two spans sum to len(a) + len(b), so as a rule one lies in
 * range and the other is negative or tiny; with inserts shorter than the two reads together both may land in range.  The caller reads the
 * library's orientation off where the mass lies: the row with the largest n_in, its mass away from the first few bins.
 * params->flag, filters, filterd and mark_mismatch are not looked at: the fill is flag 0's, and there is no reverse pass, traceback or
 * CIGAR in this call.  hist is [3][max_span + 1] 32-bit counts, row index SSW_GPU_MATES_FR / _RF / _FF; on success every entry is written.
 * On the device: the forward fill of ssw_gpu_align_windows_best over all candidates (the fallback at flag 0 for those outside the
 * envelopes, their records uploaded beside the fill's); then k_insertstat, one 16-lane row per fragment on a bounded grid whose rows stride
 * over the fragments: two key pairs per row, the winners' digests and spans as k_matebest forms them, 32-bit integer atomic adds into
 * the bins (sums of integers: the answer does not depend on the order of arrival), the nine counters kept in registers and added once
 * per workgroup.  Nothing per fragment comes to the host.
 * Memory beyond the fill's (an output of the call, not scratch under ssw_gpu_get_budget): per candidate 48 bytes of record, 4 of slot map
 * and 16 of side table, per fragment 16 of offsets, and 3 * (max_span + 1) + 16 32-bit words of bins and counters (at most 768 KiB + 64).
 * Errors (-1 with a message, before anything is launched or written): every check of ssw_gpu_align_windows_mates_lib that applies -- a
 * NULL array, cand_off[0] != 0, a decreasing cand_off, a group over SSW_GPU_MATES_GROUP_MAX, the counts beyond 0x7fffff00, nfwd outside
 * [0, queries->count], an index or window out of range, sequences of another context --; hist or counts NULL; min_margin outside
 * 0 .. 65535; max_span outside 0 .. SSW_GPU_INSERT_SPAN_MAX.  nfrag == 0 returns 0 with hist and counts zeroed.  SSW_GPU_BUSY, the
 * context lock and the budget as for ssw_gpu_align_windows.
 * ssw_gpu_last_timing: reduce_ms is the device time of k_insertstat; the fill fields as for ssw_gpu_align_windows_mates_lib; best_flagged 0.
 * Histograms of blocks of one library simply add, entry by entry and counter by counter.
 *
 * ssw_gpu_insert_fit: one row of such a histogram (n_entries = max_span + 1 counts) to the numbers a mates call takes.  Host arithmetic
 * only: no context, no device.  mem_pestat's rule with the rounding pinned in integers; with h[d] the fragments of span d,
 *   N = sum h;  N < 10: return 1.
 *   kth(k) = the smallest d with h[0] + .. + h[d] > k;  p25, p50, p75 = kth((250 N + 499) / 1000), kth((500 N + 499) / 1000),
 *   kth((750 N + 499) / 1000) in integer division;  iqr = p75 - p25;
 *   out_lo = max(p25 - 2 iqr, 1), out_hi = min(p75 + 2 iqr, n_entries - 1);
 *   n_used, sum, sum2 = sum of h[d], d h[d], d d h[d] over out_lo <= d <= out_hi;  n_used == 0: return 1;
 *   mean = (double)sum / (double)n_used;  sd = sqrt((double)(n_used * sum2 - sum * sum) / ((double)n_used * (double)n_used)), the
 *   numerator exact in 128 bits and converted once;
 *   min_insert = max(min(p25 - 3 iqr, floor(mean - 4.0 sd + 0.499)), 1);
 *   max_insert = min(max(p75 + 3 iqr, floor(mean + 4.0 sd + 0.499)), n_entries - 1).
 * Every floating-point step is one correctly rounded IEEE double operation (no fused multiply-add), so mean and sd are the same bits on
 * every host.  Returns 0: fitted; 1: too few observations, *out zeroed except n_total; -1: a NULL argument, n_entries < 1, or
 * N >= 2^31.  A table for the model from the fit: ssw_amd.insert_model_normal (Python).
 * Not provided: a pool variant (histograms of blocks simply add); a BatchAligner method; a CLI option; MAPQ; histograms from real begin
 * positions (the flagged records' ref_begin1).
 */
#define SSW_GPU_INSERT_SPAN_MAX 65535          /* max_span + 1 <= SSW_GPU_INSERT_TABLE_MAX */
typedef struct {
	int64_t n_both;     /* fragments in which both mates have an eligible candidate */
	int64_t n_unique;   /* ... and the best of either mate passes min_margin */
	int64_t n_same;     /* ... and both bests lie on one target */
	int64_t n_in[3];    /* per orientation o: strand rule holds and 0 <= D_o <= max_span (== sum of hist[o]) */
	int64_t n_out[3];   /* per orientation o: strand rule holds, D_o outside 0 .. max_span */
} ssw_gpu_insert_counts;
int ssw_gpu_insert_hist(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* queries, const ssw_gpu_seqs* targets,
                        const int64_t* cand_off, int64_t nfrag,
                        const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                        int32_t nfwd, const ssw_gpu_params* params, int32_t min_score,
                        int32_t min_margin, int32_t max_span,
                        uint32_t* hist /* [3][max_span + 1], index SSW_GPU_MATES_FR / _RF / _FF */,
                        ssw_gpu_insert_counts* counts);
typedef struct {
	int64_t n_total, n_used;        /* N; n inside the outlier bounds */
	int32_t p25, p50, p75;          /* quartiles of the spans */
	int32_t out_lo, out_hi;         /* outlier bounds */
	uint64_t sum, sum2;             /* S1, S2 over the spans inside them */
	double mean, sd;
	int32_t min_insert, max_insert; /* the range a mates call is given */
} ssw_gpu_insert_stats;
int ssw_gpu_insert_fit(const uint32_t* hist_row, int32_t n_entries, ssw_gpu_insert_stats* out);

int ssw_gpu_last_timing(const ssw_gpu_ctx* ctx, ssw_gpu_timing* out);
/* the first min(out_size, sizeof(ssw_gpu_timing)) bytes of the record (the rest of `out`, if any, zeroed): a binary built against
   an earlier, shorter ssw_gpu_timing passes ITS sizeof and is not written past it */
int ssw_gpu_last_timing_sized(const ssw_gpu_ctx* ctx, void* out, size_t out_size);

/* Return codes of the batch calls: 0 ok; -1 failed, ssw_gpu_last_error(ctx) says why; SSW_GPU_BUSY another thread is inside this
   context (no message is written: the running call owns the error text); > 0 from ssw_gpu_search_db: the value the caller's chunk
   function returned to stop the search. */
#define SSW_GPU_BUSY (-2)
const char* ssw_gpu_strerror(int rc);

/* Scratch budget of a context in bytes (column maxima, boundary records, traceback scratch).  Default: min(64 GiB, half of the HBM that
   was free when the context was opened), or SSW_GPU_CM_BUDGET_MB -- it assumes nothing about other users of the device (HIP does not
   refuse another process's over-subscribing allocation; the failure would only show at a kernel launch).  Contexts sharing a device
   (several ranks or pool workers per GPU) should each get their share: ssw_gpu_pool_open does that for its workers.
   ssw_gpu_set_budget(ctx, 0) recomputes the default; ssw_gpu_set_budget_exclusive(ctx) is the caller's statement that the context
   has the device to itself: min(200 GiB, 60 % of the free HBM) -- the 288 GB of an MI355X then hold 3 fill launches per 100 000
   150-bp reads against 1 Mb instead of 6 (+1 %).  UNSAFE on a device that other processes use: their allocations are not refused, a later
   kernel launch of either side fails instead.  Every phase of a call, the traceback included, stays within the budget. */
int ssw_gpu_set_budget(ssw_gpu_ctx* ctx, size_t bytes);
int ssw_gpu_set_budget_exclusive(ssw_gpu_ctx* ctx);
size_t ssw_gpu_get_budget(const ssw_gpu_ctx* ctx);

/*
 * Database search with streamed results.  Every query against every target, scores and end positions only -- what the
 * reference's loop (src/main.c:462-526) computes with flag 0 -- for sizes whose result matrix does not fit anywhere at once
 * (BASELINE config 5: 50 000 x 10 000 = 5e8 alignments).  Targets are processed in chunks of `targets_per_chunk`; for every
 * chunk `fn` receives the compact records hits[q * target_count + t] of targets [target_first, target_first + target_count)
 * (valid only during the call) while the device already works on the next chunk.  fn returns 0 to go on, non-zero to stop
 * (ssw_gpu_search_db then returns that value).  params->flag must be 0.
 * Streamed (chunk i + 1 is filled while chunk i is downloaded and handed to fn) inside the database search's envelope as described at
 * ssw_gpu_align_batch: short queries on k_filldb and queries of up to 65 535 residues on the strip kernel's pair mode write one chunk
 * matrix.  NOT streamed -- every chunk then produces full records that are converted on the host, same values, no overlap -- with
 * gapO <= gapE, more than 32 letters, max(mat) > 49, a target over 65 000 columns, or a query above 640 residues (384 for n >= 26) whose
 * job does not fit half of ssw_gpu_get_budget (a longest target of roughly budget / 48 columns and more).
 */
typedef struct {
	uint16_t score1;     /* as s_align */
	uint16_t score2;
	int32_t ref_end1;
	int32_t read_end1;
	int32_t ref_end2;    /* -2: the reference returns NULL for this pair (8-bit overflow with score_size 0) */
} ssw_gpu_hit;
typedef int (*ssw_gpu_hits_fn)(void* user, int32_t target_first, int32_t target_count, const ssw_gpu_hit* hits);
int ssw_gpu_search_db(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* queries, const ssw_gpu_seqs* targets, const ssw_gpu_params* params,
                      int32_t targets_per_chunk, ssw_gpu_hits_fn fn, void* user);

/*
 * Database search, best k targets per query -- the reference's loop (src/main.c:462-526) kept to its best hits, without shipping the
 * nq x nt matrix to the host.  Target t of the whole set is ELIGIBLE for query q when its ssw_gpu_align_batch record has status 0,
 * score1 > 0 and score1 >= min_score.
 *   tidx[q * k + r]     the r-th eligible target of query q, ordered by score1 descending, then target index ascending; -1 past the last;
 *   results[q * k + r]  bit for bit the ssw_gpu_align_batch(ctx, queries, targets, t, 1, params, ...) record at row q (the caller's flag,
 *                       filters, filterd, maskLen, score_size, mark_mismatch); padding slots hold the record of an empty target (zeros,
 *                       ref_begin1 = read_begin1 = -1, cigar_off = -1);
 *   cigar_pool          (optional, malloc()ed, caller frees) the CIGARs in (q, r) order.
 * targets_per_chunk: 0 = 2048, as ssw_gpu_search_db (the answer does not depend on it).  k outside 1..SSW_GPU_TOPK_MAX, a NULL tidx /
 * results / params or sequences of another context return -1 with a message before anything is launched or written; nq == 0 returns 0;
 * nt == 0 fills every slot with padding.  Every phase stays within ssw_gpu_get_budget(ctx).
 * Inside the database search's envelope (n <= 32, max(mat) <= 49, gapO > gapE, targets up to 65 000 columns; queries of any length up to
 * 65 535 residues -- those above 640, or above 384 for n >= 26, on the strip kernel's pair mode as described at ssw_gpu_align_batch) the
 * selection runs on the device (k_topk, one launch per chunk of targets, beside the next chunk's fill), and the lists come to the host
 * once; elsewhere the chunks' full records are selected on the host -- exact, slower.  With flag != 0 the selected pairs then go through
 * the ssw_gpu_align_pairs path (whose own fast paths leave queries of 641..768 residues out).
 * ssw_gpu_last_timing: reduce_ms is the device time of the k_topk selection launches (the other fields as for the search and the pairs).
 */
#define SSW_GPU_TOPK_MAX 1024
int ssw_gpu_search_topk(ssw_gpu_ctx* ctx, const ssw_gpu_seqs* queries, const ssw_gpu_seqs* targets,
                        const ssw_gpu_params* params, int32_t k, int32_t min_score, int32_t targets_per_chunk,
                        int32_t* tidx, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words);

/*
 * Threads.  A context owns one stream set and its workspaces: ONE call at a time per context (a second thread entering
 * ssw_gpu_align_batch on a busy context gets an error, not a race).  Different contexts -- on the same or on different
 * devices -- are independent and may be driven from different threads concurrently.  The single-pair functions of ssw.h
 * use an implicit context per calling thread (devices assigned round-robin, or SSW_GPU_DEVICE), so concurrent ssw_align
 * calls on one const s_profile* are legal, as with the reference (src/ssw.c has no mutable global state).
 * Streaming callers: while a batch call runs on a context, ONE other thread may prepare the next block on the same context with the
 * ssw_gpu_seqs_* calls (upload, ASCII translation, reverse complement) and free finished sets; those run on the context's upload stream
 * and do not queue behind the batch call's kernels (ssw_test_gpu's three stages, bench.py --config 3 --full).  The context's lazily created
 * streams and its error text are guarded by a lock (round 6): the feeder thread's first upload may race the first batch call.
 */

/*
 * Several devices, one batch: per-GPU work queues (the loop of reference src/main.c:462-526 spread over a node).
 * A pool holds one worker (context + host thread) per entry of `devices`; the target set is replicated on every worker's
 * device, the queries stay on the host and are pulled in blocks of `block` reads from a shared queue, each block is
 * uploaded and aligned by whichever worker is free, and every record lands in its own slot results[q * target_count + t]
 * -- output order does not depend on which device did what.  No inter-device traffic at all.
 */
typedef struct ssw_gpu_pool ssw_gpu_pool;
/* devices == NULL: one worker per visible device (n ignored); else n entries, an index may repeat (several workers on one
   device share it through separate streams). */
ssw_gpu_pool* ssw_gpu_pool_open(const int* devices, int n);      /* NULL on failure: ssw_gpu_last_error(NULL) */
void ssw_gpu_pool_close(ssw_gpu_pool* pool);
int ssw_gpu_pool_size(const ssw_gpu_pool* pool);
size_t ssw_gpu_pool_budget(const ssw_gpu_pool* pool, int worker);   /* scratch budget of that worker's context: workers sharing a device share its HBM */
const char* ssw_gpu_pool_last_error(const ssw_gpu_pool* pool);
int ssw_gpu_pool_set_targets(ssw_gpu_pool* pool, const int8_t* codes, const int64_t* offsets, int32_t count);
int ssw_gpu_pool_align(ssw_gpu_pool* pool, const int8_t* qcodes, const int64_t* qoffsets, int32_t nq, int32_t block,
                       int32_t target_first, int32_t target_count, const ssw_gpu_params* params,
                       ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words);
/* ssw_gpu_search_topk over the pool's target set: blocks of `block` queries (0: a few per worker) go to whichever worker is free, rows
   tidx[q * k ..] / results[q * k ..] land in place, CIGAR offsets are rebased into one pool in block order -- the same output as one
   context's ssw_gpu_search_topk over all queries (targets_per_chunk: the default) */
int ssw_gpu_pool_search_topk(ssw_gpu_pool* pool, const int8_t* qcodes, const int64_t* qoffsets, int32_t nq, int32_t block,
                             const ssw_gpu_params* params, int32_t k, int32_t min_score, int32_t* tidx, ssw_gpu_result* results,
                             uint32_t** cigar_pool, int64_t* cigar_words);
/*
 * The window entry points over the pool: ssw_gpu_align_windows and ssw_gpu_align_windows_topk with the pool's resident target set
 * (ssw_gpu_pool_set_targets, replicated once per worker; tidx / tbeg / tlen index it) and reads that stay on the host, as for
 * ssw_gpu_pool_align.  with_revcomp != 0: qidx in [nq, 2 nq) names the reverse complement of read qidx - nq, the convention of
 * ssw_gpu_seqs_with_revcomp -- a worker builds the reverse complements it needs on its device, the caller never does.
 * Output: bit for bit what ONE context gives for ssw_gpu_align_windows / ssw_gpu_align_windows_topk over all the reads (with_revcomp:
 * over ssw_gpu_seqs_with_revcomp of them) -- results, pos, n_eligible, cigar_off and the words of the CIGAR pool -- whatever the number
 * of workers, whichever worker took which block, and whatever `block` is.
 * Blocks: contiguous ranges, in order, of pairs (align_windows: `block` pairs each) or of WHOLE groups (topk: a block takes groups until
 * it holds at least `block` candidates; always at least one group; empty groups belong to the block they fall into).  block <= 0: a few
 * blocks per worker by candidate count, ceil(candidates / (4 x workers)), but at least 16 384 candidates per block -- below that the
 * host planning of a window call outweighs its kernels.  A worker uploads only the distinct forward reads its block names, in ascending read
 * index, renumbers the block's qidx to them (forward read j of m is j, its reverse complement m + j; ssw_gpu_seqs_with_revcomp only if
 * the block names a reverse strand), rebases cand_off to the block and passes the slices of tidx / tbeg / tlen / pos / n_eligible /
 * results in place.  The blocks' CIGAR pools are concatenated in block order, cigar_off rebased: pair order, or (group, rank) order.
 * Errors (-1, text in ssw_gpu_pool_last_error; before any worker starts and before any output is written; the pair or group is named
 * by its index in the CALLER's arrays): a NULL array, no target set, k outside 1..SSW_GPU_GROUP_TOPK_MAX, cand_off[0] != 0 or a
 * decreasing cand_off, qidx outside [0, nq) -- [0, 2 nq) with with_revcomp --, tidx out of range, tbeg < 0, tlen < 0, a window past the
 * end of its target.  npairs == 0 / ngroups == 0 return 0 with *cigar_words = 0.  A failure inside a worker stops the hand-out and
 * reports worker, device and the block's range of pairs or groups.  ssw_gpu_pool_stats: blocks taken, `queries` = distinct reads
 * uploaded (summed over the blocks), cells, busy milliseconds.
 * There is no pool variant of ssw_gpu_align_windows_best: ssw_gpu_pool_align_windows_topk answers it -- k = 1 gives `best` and its
 * record; k = 2 with max_drop < 0 gives `second` in pos[2 g + 1] and second_score1 in results[2 g + 1].score1; n_eligible is returned
 * as it is.
 */
int ssw_gpu_pool_align_windows(ssw_gpu_pool* pool,
        const int8_t* qcodes, const int64_t* qoffsets, int32_t nq, int with_revcomp,
        const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen, int64_t npairs,
        int64_t block, const ssw_gpu_params* params,
        ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words);
int ssw_gpu_pool_align_windows_topk(ssw_gpu_pool* pool,
        const int8_t* qcodes, const int64_t* qoffsets, int32_t nq, int with_revcomp,
        const int64_t* cand_off, int64_t ngroups,
        const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
        int64_t block, const ssw_gpu_params* params, int32_t k, int32_t min_score, int32_t max_drop,
        int32_t* pos, int32_t* n_eligible, ssw_gpu_result* results,
        uint32_t** cigar_pool, int64_t* cigar_words);
/*
 * ssw_gpu_align_windows_mates_lib over the pool, on the conventions above: the pool's target set, reads on the host, with_revcomp.
 * Output: bit for bit what ONE context gives for ssw_gpu_align_windows_mates_lib over all the reads with nfwd = nq (with_revcomp: over
 * ssw_gpu_seqs_with_revcomp of them; without it everything is on the plus strand) -- sel, both records per fragment, cigar_off and the
 * words of the CIGAR pool, in (fragment, mate) order -- whatever the workers, whichever took which block, and whatever `block` is.
 * Blocks: contiguous runs of WHOLE fragments; a block takes fragments until it holds at least `block` candidates, always at least one,
 * empty fragments stay in the block they fall into; block <= 0 as for the other window calls, by candidate count.  A worker uploads the
 * distinct forward reads of its block (m of them), renumbers qidx, rebases the block's 2 cnt + 1 offsets and calls the single-context
 * entry point with nfwd = m; sel + f0 and results + 2 f0 are written in place.
 * Errors (-1, text in ssw_gpu_pool_last_error, before any worker starts and before any output is written, naming the CALLER's fragment,
 * mate or pair): every check of ssw_gpu_align_windows_mates_lib over the whole list -- a NULL array, no target set, cand_off[0] != 0, a
 * decreasing cand_off, a group over SSW_GPU_MATES_GROUP_MAX, min_insert < 0 or > max_insert, unpaired_penalty outside 0 .. 65535, an
 * orientation outside 0 .. 2 -- and the index and window checks of the other pool window calls.  nfrag == 0 returns 0 with
 * *cigar_words = 0.  A failure inside a worker names worker, device and the block's range of fragments.  ssw_gpu_pool_stats as above.
 */
int ssw_gpu_pool_align_windows_mates(ssw_gpu_pool* pool,
        const int8_t* qcodes, const int64_t* qoffsets, int32_t nq, int with_revcomp,
        const int64_t* cand_off, int64_t nfrag,
        const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
        int64_t block, const ssw_gpu_params* params, int32_t min_score,
        int32_t min_insert, int32_t max_insert, int32_t unpaired_penalty, int32_t orientation,
        ssw_gpu_mates* sel, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words);
/*
 * ssw_gpu_pool_align_windows_mates under a pair model (ssw_gpu_pair_model above): bit for bit what ONE context gives for
 * ssw_gpu_align_windows_mates_model over all the reads, whatever the workers and `block`.  model->insert_penalty is one read-only host
 * array shared by the workers for the length of the call; every worker's context makes its own device copy per block (2 bytes per entry).
 * Errors as ssw_gpu_pool_align_windows_mates, over the whole list before any worker starts, and: model == NULL; a non-NULL table with
 * max_insert - min_insert + 1 > SSW_GPU_INSERT_TABLE_MAX.
 */
int ssw_gpu_pool_align_windows_mates_model(ssw_gpu_pool* pool,
        const int8_t* qcodes, const int64_t* qoffsets, int32_t nq, int with_revcomp,
        const int64_t* cand_off, int64_t nfrag,
        const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
        int64_t block, const ssw_gpu_params* params, int32_t min_score,
        const ssw_gpu_pair_model* model,
        ssw_gpu_mates* sel, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words);
/* per worker, accumulated over the last pool call: blocks taken, reads uploaded, DP cells (readLen x refLen), device milliseconds */
typedef struct { int32_t device; int64_t blocks; int64_t queries; int64_t cells; double busy_ms; } ssw_gpu_pool_stat;
int ssw_gpu_pool_stats(const ssw_gpu_pool* pool, int worker, ssw_gpu_pool_stat* out);

/* Page-locked host memory for result arrays (optional): a database search returns nq x nt records, and their download
   runs at PCIe rate only into pinned pages.  Any host pointer is accepted by ssw_gpu_align_batch; this one is faster. */
void* ssw_gpu_host_alloc(ssw_gpu_ctx* ctx, size_t bytes);
void ssw_gpu_host_free(ssw_gpu_ctx* ctx, void* p);

/* (Diagnostics -- lane self-test, VALU issue probe, test-hook query -- are declared in include/ssw_gpu_diag.h and exist only in
   libssw_hooks.so: the product library exports the reference's symbols and the batch ABI above, one by one, in libssw.map.) */

/* Single-pair callers (ssw_align) get an implicit context per calling thread; a thread that ends parks its context for the next new caller
   thread (at most 4 stay parked).  This closes every parked context now -- their streams, scratch pools and resident target copies -- and
   returns how many were closed.  Call it from a live thread after a burst of short-lived caller threads. */
int ssw_gpu_release_parked(void);

/* Convert one batch record into a heap s_align (align_destroy()-compatible), copying its CIGAR. */
s_align* ssw_gpu_result_to_align(const ssw_gpu_result* r, const uint32_t* cigar_pool);

#ifdef __cplusplus
}
#endif
#endif /* SSW_GPU_H */
