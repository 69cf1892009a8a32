/*
 * ssw_pool.c -- several devices, one batch: the per-GPU work queues of SURVEY 8e (north_star: "batches of independent
 * query x reference alignments shard trivially across the 8 GPUs of one node; no RCCL needed; per-GPU work queues only").
 *
 * What it replaces in the reference: the read loop of src/main.c:462-526 (one ssw_init + one ssw_align per target per read,
 * on one core).  Here a pool owns one worker per device -- a context (its own streams and workspaces, include/ssw_gpu.h)
 * plus one host thread for the duration of a call -- the target set is uploaded once to every device, and blocks of work
 * are handed out through one atomic counter.  A block is a contiguous range of UNITS -- reads (ssw_gpu_pool_align,
 * ssw_gpu_pool_search_topk), pairs (ssw_gpu_pool_align_windows), groups (ssw_gpu_pool_align_windows_topk) or fragments
 * (ssw_gpu_pool_align_windows_mates) --, a unit owns `width` consecutive record slots, CIGAR pools are concatenated in block order afterwards, so the output is identical to
 * the single-context call over the whole list.
 * Uses only the public batch ABI; host code, plain C.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ssw_gpu.h"

typedef struct {
	ssw_gpu_ctx* ctx;
	ssw_gpu_seqs* targets;
	int device;
	ssw_gpu_pool_stat st;
} pool_worker;

struct ssw_gpu_pool {
	int n;
	pool_worker* w;
	int32_t tcount;
	int64_t* toff;               /* host copy of the target offsets (tcount + 1): the window calls check every window before a worker starts */
	char err[512];
};

typedef struct { uint32_t* words; int64_t n; } block_cigars;

/* what a worker thread keeps from block to block of a window call (DESIGN "Window lists over a pool"): the read -> local index map
   (-1 outside a block) and the block's copies -- its distinct reads, its renumbered qidx, its rebased cand_off */
typedef struct {
	int32_t* map;                /* nq entries */
	int32_t* reads; int64_t cap_reads;
	int32_t* lq; int64_t cap_lq;
	int64_t* loff; int64_t cap_loff;
	int8_t* codes; int64_t cap_codes;
	int64_t* lco; int64_t cap_groups;
} win_scratch;

/* one pool call, shared by its worker threads */
typedef struct pool_call pool_call;
struct pool_call {
	ssw_gpu_pool* pool;
	const int8_t* qcodes; const int64_t* qoff; int32_t nq;
	const ssw_gpu_params* prm;
	ssw_gpu_result* results;
	/* the queue: nunits units in nblocks contiguous blocks -- `block` units each (the last one shorter), or, with bstart, units
	   [bstart[b], bstart[b + 1]) --; a unit owns `width` records */
	int64_t nunits, block, nblocks, width;
	int64_t* bstart;
	const char* unit;            /* "reads", "pairs", "groups", "fragments": how a failure names its block */
	/* one block on one worker: 0, or -1 with the reason in the worker's context (or in *why, a host-side failure); *uploaded: reads sent */
	int (*run)(pool_call* k, pool_worker* w, win_scratch* ws, int64_t b, int64_t u0, int64_t cnt, int64_t* uploaded, const char** why);
	block_cigars* cig;           /* per block */
	int want_cigars;
	/* read blocks */
	int32_t tfirst, tcount;
	int32_t topk, min_score;     /* topk > 0: ssw_gpu_search_topk per block, rows of topk slots (tidx + results) */
	int32_t* tidx;
	/* window lists */
	const int64_t* cand_off;     /* groups (ssw_gpu_align_windows_topk, _mates) or NULL (ssw_gpu_align_windows: a unit is a pair) */
	int64_t gpu;                 /* groups per unit: 1, or 2 for ssw_gpu_align_windows_mates (a unit is a fragment: its two mates' groups) */
	const int32_t* wq; const int32_t* wt; const int64_t* wbeg; const int32_t* wlen;
	int32_t wk, max_drop;
	int32_t* pos; int32_t* n_eligible;
	ssw_gpu_mates* mates;        /* ssw_gpu_align_windows_mates: one selection per fragment, and the rule's arguments */
	int32_t min_insert, max_insert, unpaired_penalty, orientation;
	const uint16_t* ins_pen;     /* pair model: the caller's penalty table, read-only and shared by the workers (each context uploads its own copy); NULL: the flat rule */
	int64_t next;                /* next block index (atomic) */
	int failed;                  /* first failure stops the hand-out (atomic) */
	pthread_mutex_t err_lock;
};

typedef struct { pool_call* call; int widx; } pool_thread_arg;

static void block_range(const pool_call* k, int64_t b, int64_t* u0, int64_t* cnt)
{
	if (k->bstart) { *u0 = k->bstart[b]; *cnt = k->bstart[b + 1] - k->bstart[b]; return; }
	*u0 = b * k->block;
	*cnt = k->nunits - *u0 < k->block ? k->nunits - *u0 : k->block;
}

/* a block of reads against the resident targets */
static int run_reads(pool_call* k, pool_worker* w, win_scratch* ws, int64_t b, int64_t q0, int64_t cnt, int64_t* uploaded, const char** why)
{
	(void)ws; (void)why;
	ssw_gpu_seqs* Q = ssw_gpu_seqs_upload(w->ctx, k->qcodes, k->qoff + q0, (int32_t)cnt);   /* offsets are taken relative to their first entry */
	if (!Q) return -1;
	int rc;
	if (k->topk > 0)
		rc = ssw_gpu_search_topk(w->ctx, Q, w->targets, k->prm, k->topk, k->min_score, 0, k->tidx + q0 * k->topk,
		                         k->results + q0 * k->topk, k->want_cigars ? &k->cig[b].words : 0, k->want_cigars ? &k->cig[b].n : 0);
	else
		rc = ssw_gpu_align_batch(w->ctx, Q, w->targets, k->tfirst, k->tcount, k->prm, k->results + q0 * k->tcount,
		                         k->want_cigars ? &k->cig[b].words : 0, k->want_cigars ? &k->cig[b].n : 0);
	ssw_gpu_seqs_free(Q);
	*uploaded = cnt;
	return rc;
}

static int cmp_i32(const void* a, const void* b)
{
	const int32_t x = *(const int32_t*)a, y = *(const int32_t*)b;
	return x < y ? -1 : x > y;
}

static int grow(void** p, int64_t* cap, int64_t need, size_t elem)
{
	if (need <= *cap) return 0;
	free(*p);
	*cap = need + need / 4 + 16;
	*p = malloc(elem * (size_t)*cap);
	if (!*p) { *cap = 0; return -1; }
	return 0;
}

/* a block of a window list: pairs [u0, u0 + cnt), or groups [u0, u0 + cnt) with their candidates, or fragments [u0, u0 + cnt) with the
   candidates of their 2 cnt groups.  The block's candidates name arbitrary reads on either strand: the worker uploads the DISTINCT forward reads among them in ascending read index (m of them), builds their
   reverse complements on its device only if the block names one, and renumbers qidx to that set -- forward read j is j, its reverse
   complement m + j -- so that a candidate is on the minus strand iff its local index is >= m, the nfwd a block of fragments is called
   with.  tidx / tbeg / tlen and the output slices are the caller's arrays in place. */
static int run_windows(pool_call* k, pool_worker* w, win_scratch* ws, int64_t b, int64_t u0, int64_t cnt, int64_t* uploaded, const char** why)
{
	const int64_t g0 = u0 * k->gpu, ng = cnt * k->gpu;      /* (the block's groups; gpu is 1 without cand_off) */
	const int64_t p0 = k->cand_off ? k->cand_off[g0] : u0, p1 = k->cand_off ? k->cand_off[g0 + ng] : u0 + cnt, np = p1 - p0;
	const int32_t nq = k->nq;
	*why = "out of host memory (window block)";
	if (!ws->map) {
		ws->map = (int32_t*)malloc(sizeof(int32_t) * ((size_t)nq + 1));
		if (!ws->map) return -1;
		memset(ws->map, 0xff, sizeof(int32_t) * ((size_t)nq + 1));
	}
	if (grow((void**)&ws->reads, &ws->cap_reads, np, sizeof(int32_t)) || grow((void**)&ws->lq, &ws->cap_lq, np, sizeof(int32_t))) return -1;
	int32_t m = 0;
	int rev = 0, ascending = 1;
	for (int64_t i = p0; i < p1; ++i) {
		int32_t r = k->wq[i];
		if (r >= nq) { r -= nq; rev = 1; }
		if (ws->map[r] < 0) {
			ws->map[r] = 0;
			if (m > 0 && ws->reads[m - 1] > r) ascending = 0;
			ws->reads[m++] = r;
		}
	}
	if (!ascending) qsort(ws->reads, (size_t)m, sizeof(int32_t), cmp_i32);
	int64_t total = 0;
	for (int32_t j = 0; j < m; ++j) total += k->qoff[ws->reads[j] + 1] - k->qoff[ws->reads[j]];
	int rc = -1;
	ssw_gpu_seqs* F = 0; ssw_gpu_seqs* Q = 0;
	if (grow((void**)&ws->loff, &ws->cap_loff, (int64_t)m + 1, sizeof(int64_t)) || grow((void**)&ws->codes, &ws->cap_codes, total + 1, 1) ||
	    (k->cand_off && grow((void**)&ws->lco, &ws->cap_groups, ng + 1, sizeof(int64_t)))) {
		for (int32_t j = 0; j < m; ++j) ws->map[ws->reads[j]] = -1;
		return -1;
	}
	ws->loff[0] = 0;
	for (int32_t j = 0; j < m; ++j) {
		const int32_t r = ws->reads[j];
		const int64_t len = k->qoff[r + 1] - k->qoff[r];
		ws->map[r] = j;
		if (len > 0) memcpy(ws->codes + ws->loff[j], k->qcodes + k->qoff[r], (size_t)len);
		ws->loff[j + 1] = ws->loff[j] + len;
	}
	for (int64_t i = p0; i < p1; ++i) {
		const int32_t q = k->wq[i];
		ws->lq[i - p0] = q >= nq ? m + ws->map[q - nq] : ws->map[q];
	}
	for (int32_t j = 0; j < m; ++j) ws->map[ws->reads[j]] = -1;
	*why = 0;
	F = ssw_gpu_seqs_upload(w->ctx, ws->codes, ws->loff, m);
	if (!F) return -1;
	if (rev) {
		Q = ssw_gpu_seqs_with_revcomp(w->ctx, F);
		ssw_gpu_seqs_free(F);
		if (!Q) return -1;
	} else
		Q = F;
	uint32_t** const cw = k->want_cigars ? &k->cig[b].words : 0;
	int64_t* const cn = k->want_cigars ? &k->cig[b].n : 0;
	if (k->cand_off) {
		for (int64_t g = 0; g <= ng; ++g) ws->lco[g] = k->cand_off[g0 + g] - p0;
		if (k->mates && k->ins_pen) {
			const ssw_gpu_pair_model pm = { k->min_insert, k->max_insert, k->unpaired_penalty, k->orientation, k->ins_pen };
			rc = ssw_gpu_align_windows_mates_model(w->ctx, Q, w->targets, ws->lco, cnt, ws->lq, k->wt + p0, k->wbeg + p0, k->wlen + p0, m, k->prm,
			                                       k->min_score, &pm, k->mates + u0, k->results + 2 * u0, cw, cn);
		} else if (k->mates)
			rc = ssw_gpu_align_windows_mates_lib(w->ctx, Q, w->targets, ws->lco, cnt, ws->lq, k->wt + p0, k->wbeg + p0, k->wlen + p0, m, k->prm,
			                                     k->min_score, k->min_insert, k->max_insert, k->unpaired_penalty, k->orientation, k->mates + u0,
			                                     k->results + 2 * u0, cw, cn);
		else
			rc = ssw_gpu_align_windows_topk(w->ctx, Q, w->targets, ws->lco, cnt, ws->lq, k->wt + p0, k->wbeg + p0, k->wlen + p0, k->prm, k->wk,
			                                k->min_score, k->max_drop, k->pos + u0 * k->wk, k->n_eligible + u0, k->results + u0 * k->wk, cw, cn);
	} else
		rc = ssw_gpu_align_windows(w->ctx, Q, w->targets, ws->lq, k->wt + p0, k->wbeg + p0, k->wlen + p0, np, k->prm, k->results + u0, cw, cn);
	ssw_gpu_seqs_free(Q);
	*uploaded = m;
	return rc;
}

static void* pool_thread(void* argp)
{
	pool_thread_arg* a = (pool_thread_arg*)argp;
	pool_call* k = a->call;
	pool_worker* w = &k->pool->w[a->widx];
	win_scratch ws; memset(&ws, 0, sizeof ws);
	for (;;) {
		if (__atomic_load_n(&k->failed, __ATOMIC_ACQUIRE)) break;
		const int64_t b = __atomic_fetch_add(&k->next, 1, __ATOMIC_RELAXED);
		if (b >= k->nblocks) break;
		int64_t u0, cnt, uploaded = 0;
		const char* why = 0;
		block_range(k, b, &u0, &cnt);
		if (k->run(k, w, &ws, b, u0, cnt, &uploaded, &why)) {
			pthread_mutex_lock(&k->err_lock);
			if (!__atomic_exchange_n(&k->failed, 1, __ATOMIC_ACQ_REL))
				snprintf(k->pool->err, sizeof k->pool->err, "worker %d (device %d), %s %lld..%lld: %s", a->widx, w->device, k->unit, (long long)u0,
				         (long long)(u0 + cnt - 1), why ? why : ssw_gpu_last_error(w->ctx));
			pthread_mutex_unlock(&k->err_lock);
			break;
		}
		ssw_gpu_timing tm;
		if (ssw_gpu_last_timing(w->ctx, &tm) == 0) { w->st.cells += tm.cells; w->st.busy_ms += tm.total_ms; }
		w->st.blocks++; w->st.queries += uploaded;
	}
	free(ws.map); free(ws.reads); free(ws.lq); free(ws.loff); free(ws.codes); free(ws.lco);
	return 0;
}

ssw_gpu_pool* ssw_gpu_pool_open(const int* devices, int n)
{
	const int ndev = ssw_gpu_device_count();
	if (ndev < 1) { (void)ssw_gpu_open(0); return 0; }          /* leaves the "no device" message in ssw_gpu_last_error(NULL) */
	if (!devices) n = ndev;
	if (n < 1 || n > 1024) return 0;
	ssw_gpu_pool* p = (ssw_gpu_pool*)calloc(1, sizeof *p);
	if (!p) return 0;
	p->w = (pool_worker*)calloc((size_t)n, sizeof(pool_worker));
	if (!p->w) { free(p); return 0; }
	p->n = n;
	for (int i = 0; i < n; ++i) {
		p->w[i].device = devices ? devices[i] : i;
		p->w[i].st.device = p->w[i].device;
		p->w[i].ctx = ssw_gpu_open(p->w[i].device);
		if (!p->w[i].ctx) { ssw_gpu_pool_close(p); return 0; }   /* the reason stays in ssw_gpu_last_error(NULL) */
	}
	/* workers that share a device share its HBM: every context sized its scratch budget from what was free when IT was opened
	   (half of it) -- divide by the number of workers on that device (an explicit SSW_GPU_CM_BUDGET_MB is per context and kept) */
	if (!getenv("SSW_GPU_CM_BUDGET_MB"))
		for (int i = 0; i < n; ++i) {
			int same = 0;
			for (int j = 0; j < n; ++j) if (p->w[j].device == p->w[i].device) ++same;
			if (same > 1) ssw_gpu_set_budget(p->w[i].ctx, ssw_gpu_get_budget(p->w[i].ctx) / (size_t)same);
		}
	return p;
}

void ssw_gpu_pool_close(ssw_gpu_pool* p)
{
	if (!p) return;
	for (int i = 0; i < p->n; ++i) {
		if (p->w[i].targets) ssw_gpu_seqs_free(p->w[i].targets);
		if (p->w[i].ctx) ssw_gpu_close(p->w[i].ctx);
	}
	free(p->toff); free(p->w); free(p);
}

int ssw_gpu_pool_size(const ssw_gpu_pool* p) { return p ? p->n : 0; }
size_t ssw_gpu_pool_budget(const ssw_gpu_pool* p, int worker) { return p && worker >= 0 && worker < p->n ? ssw_gpu_get_budget(p->w[worker].ctx) : 0; }
const char* ssw_gpu_pool_last_error(const ssw_gpu_pool* p) { return p ? p->err : ssw_gpu_last_error(0); }

static void pool_drop_targets(ssw_gpu_pool* p)
{
	for (int j = 0; j < p->n; ++j) if (p->w[j].targets) { ssw_gpu_seqs_free(p->w[j].targets); p->w[j].targets = 0; }
	free(p->toff); p->toff = 0;
	p->tcount = 0;
}

int ssw_gpu_pool_set_targets(ssw_gpu_pool* p, const int8_t* codes, const int64_t* offsets, int32_t count)
{
	if (!p || !offsets || count < 0) return -1;
	int64_t* toff = (int64_t*)malloc(sizeof(int64_t) * ((size_t)count + 1));
	if (!toff) { snprintf(p->err, sizeof p->err, "out of host memory (target offsets)"); pool_drop_targets(p); return -1; }
	for (int32_t i = 0; i <= count; ++i) toff[i] = offsets[i] - offsets[0];
	for (int i = 0; i < p->n; ++i) {
		if (p->w[i].targets) { ssw_gpu_seqs_free(p->w[i].targets); p->w[i].targets = 0; }
		p->w[i].targets = ssw_gpu_seqs_upload(p->w[i].ctx, codes, offsets, count);
		if (!p->w[i].targets) {
			snprintf(p->err, sizeof p->err, "worker %d (device %d): %s", i, p->w[i].device, ssw_gpu_last_error(p->w[i].ctx));
			/* all or nothing: a pool with the new targets on some workers and the old count would answer with mixed data */
			pool_drop_targets(p);
			free(toff);
			return -1;
		}
	}
	free(p->toff);
	p->toff = toff;
	p->tcount = count;
	return 0;
}

int ssw_gpu_pool_stats(const ssw_gpu_pool* p, int worker, ssw_gpu_pool_stat* out)
{
	if (!p || !out || worker < 0 || worker >= p->n) return -1;
	*out = p->w[worker].st;
	return 0;
}

static void pool_reset_stats(ssw_gpu_pool* p)
{
	for (int i = 0; i < p->n; ++i) { const int dev = p->w[i].st.device; memset(&p->w[i].st, 0, sizeof p->w[i].st); p->w[i].st.device = dev; }
}

/* the queue of one call: the blocks of `kk` (nunits, width, run, unit and either block or bstart / nblocks set by the caller) over the
   workers, then one CIGAR pool in block order */
static int pool_run(ssw_gpu_pool* p, pool_call* kk, uint32_t** cigar_pool, int64_t* cigar_words);

/* blocks of `block` reads (0: a few blocks per worker -- the tail is one block, the upload of a block hides behind the others' compute) */
static int pool_run_reads(ssw_gpu_pool* p, pool_call* k, int32_t block, int32_t width, uint32_t** cigar_pool, int64_t* cigar_words)
{
	const int32_t nq = k->nq;
	if (block < 1) {
		block = (nq + 4 * p->n - 1) / (4 * p->n);
		if (block < 256) block = 256;
	}
	if (block > nq) block = nq;
	k->nunits = nq; k->block = block; k->width = width; k->run = run_reads; k->unit = "reads";
	return pool_run(p, k, cigar_pool, cigar_words);
}

int ssw_gpu_pool_align(ssw_gpu_pool* p, const int8_t* qcodes, const int64_t* qoffsets, int32_t nq, int32_t block,
                       int32_t target_first, int32_t target_count, const ssw_gpu_params* prm,
                       ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!p) return -1;
	if (cigar_pool) *cigar_pool = 0;
	if (cigar_words) *cigar_words = 0;
	if (!qoffsets || nq < 0 || !prm || !results) { snprintf(p->err, sizeof p->err, "pool_align: bad arguments"); return -1; }
	if (!p->w[0].targets) { snprintf(p->err, sizeof p->err, "pool_align: no target set (ssw_gpu_pool_set_targets)"); return -1; }
	if (target_first < 0 || target_count < 0 || target_first + target_count > p->tcount) { snprintf(p->err, sizeof p->err, "pool_align: target range out of bounds"); return -1; }
	pool_reset_stats(p);
	if (nq == 0 || target_count == 0) return 0;
	pool_call k; memset(&k, 0, sizeof k);
	k.qcodes = qcodes; k.qoff = qoffsets; k.nq = nq; k.tfirst = target_first; k.tcount = target_count; k.prm = prm; k.results = results;
	return pool_run_reads(p, &k, block, target_count, cigar_pool, cigar_words);
}

int ssw_gpu_pool_search_topk(ssw_gpu_pool* p, const int8_t* qcodes, const int64_t* qoffsets, int32_t nq, int32_t block,
                             const ssw_gpu_params* prm, int32_t k, int32_t min_score, int32_t* tidx, ssw_gpu_result* results,
                             uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!p) return -1;
	if (!qoffsets || nq < 0 || !prm || !prm->mat || !tidx || !results) { snprintf(p->err, sizeof p->err, "pool_search_topk: bad arguments"); return -1; }
	if (k < 1 || k > SSW_GPU_TOPK_MAX) { snprintf(p->err, sizeof p->err, "pool_search_topk: k must be 1 .. SSW_GPU_TOPK_MAX"); return -1; }
	if (!p->w[0].targets) { snprintf(p->err, sizeof p->err, "pool_search_topk: no target set (ssw_gpu_pool_set_targets)"); return -1; }
	if (cigar_pool) *cigar_pool = 0;
	if (cigar_words) *cigar_words = 0;
	pool_reset_stats(p);
	if (nq == 0) return 0;
	pool_call c; memset(&c, 0, sizeof c);
	c.qcodes = qcodes; c.qoff = qoffsets; c.nq = nq; c.tfirst = 0; c.tcount = p->tcount; c.prm = prm; c.results = results;
	c.topk = k; c.min_score = min_score; c.tidx = tidx;
	return pool_run_reads(p, &c, block, k, cigar_pool, cigar_words);
}

/* ------------------------------------------------------------------------------------------------
 * Window lists over the pool (ssw_gpu_pool_align_windows, ssw_gpu_pool_align_windows_topk)
 * ------------------------------------------------------------------------------------------------ */

/* candidates per block when the caller leaves it to the pool: a few blocks per worker, but no block so small that the per-call host work
   of the window entry points (plan, sort, job list) outweighs its kernels */
#define POOL_WINDOWS_BLOCK_FLOOR 16384

static int64_t windows_auto_block(const ssw_gpu_pool* p, int64_t np)
{
	int64_t block = (np + 4 * (int64_t)p->n - 1) / (4 * (int64_t)p->n);
	return block < POOL_WINDOWS_BLOCK_FLOOR ? POOL_WINDOWS_BLOCK_FLOOR : block;
}

/* the checks of windows_check (ssw_host.c) over the WHOLE list, with the caller's indices in the message: a worker's own check would
   name a block-local pair of block-local reads */
static int pool_windows_check(ssw_gpu_pool* p, const char* who, int32_t nq, int with_revcomp, const int32_t* qidx, const int32_t* tidx,
                              const int64_t* tbeg, const int32_t* tlen, int64_t np)
{
	const int64_t qlim = with_revcomp ? 2 * (int64_t)nq : nq;
	for (int64_t i = 0; i < np; ++i) {
		if (qidx[i] < 0 || qidx[i] >= qlim || tidx[i] < 0 || tidx[i] >= p->tcount) {
			snprintf(p->err, sizeof p->err, "%s: index out of range (pair %lld: query %d of %lld, target %d of %d)", who, (long long)i, qidx[i],
			         (long long)qlim, tidx[i], p->tcount);
			return -1;
		}
		const int64_t tl = p->toff[tidx[i] + 1] - p->toff[tidx[i]];
		if (tbeg[i] < 0 || tlen[i] < 0 || tbeg[i] > tl || (int64_t)tlen[i] > tl - tbeg[i]) {
			snprintf(p->err, sizeof p->err, "%s: window out of range (pair %lld: columns [%lld, %lld + %d) of target %d, which has %lld)", who,
			         (long long)i, (long long)tbeg[i], (long long)tbeg[i], tlen[i], tidx[i], (long long)tl);
			return -1;
		}
	}
	return 0;
}

int ssw_gpu_pool_align_windows(ssw_gpu_pool* p, const int8_t* qcodes, const int64_t* qoffsets, int32_t nq, int with_revcomp,
                               const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen, int64_t npairs,
                               int64_t block, const ssw_gpu_params* prm,
                               ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!p) return -1;
	if (cigar_pool) *cigar_pool = 0;
	if (cigar_words) *cigar_words = 0;
	if (!qoffsets || nq < 0 || npairs < 0 || !prm || !prm->mat || (npairs > 0 && (!qidx || !tidx || !tbeg || !tlen || !results))) {
		snprintf(p->err, sizeof p->err, "pool_align_windows: NULL argument");
		return -1;
	}
	if (!p->w[0].targets || !p->toff) { snprintf(p->err, sizeof p->err, "pool_align_windows: no target set (ssw_gpu_pool_set_targets)"); return -1; }
	if (pool_windows_check(p, "pool_align_windows", nq, with_revcomp, qidx, tidx, tbeg, tlen, npairs)) return -1;
	pool_reset_stats(p);
	if (npairs == 0) return 0;
	pool_call k; memset(&k, 0, sizeof k);
	k.qcodes = qcodes; k.qoff = qoffsets; k.nq = nq; k.prm = prm; k.results = results;
	k.wq = qidx; k.wt = tidx; k.wbeg = tbeg; k.wlen = tlen;
	k.nunits = npairs; k.block = block > 0 ? block : windows_auto_block(p, npairs);
	if (k.block > npairs) k.block = npairs;
	k.gpu = 1; k.width = 1; k.run = run_windows; k.unit = "pairs";
	return pool_run(p, &k, cigar_pool, cigar_words);
}

/* groups in blocks: a block takes whole units of `gpu` groups each (a group, or the two groups of a fragment), in order, until it holds at
   least `block` candidates -- at least one unit, empty ones included.  Writes the first unit of every block and nu at the end into
   bstart (when given) -> the number of blocks */
static int64_t cut_groups(const int64_t* cand_off, int64_t nu, int64_t gpu, int64_t block, int64_t* bstart)
{
	int64_t nb = 0, u = 0;
	while (u < nu) {
		if (bstart) bstart[nb] = u;
		const int64_t c0 = cand_off[u * gpu];
		++u;
		while (u < nu && cand_off[u * gpu] - c0 < block) ++u;
		++nb;
	}
	if (bstart) bstart[nb] = nu;
	return nb;
}

int ssw_gpu_pool_align_windows_topk(ssw_gpu_pool* p, const int8_t* qcodes, const int64_t* qoffsets, int32_t nq, int with_revcomp,
                                    const int64_t* cand_off, int64_t ngroups,
                                    const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                                    int64_t block, const ssw_gpu_params* prm, int32_t k, int32_t min_score, int32_t max_drop,
                                    int32_t* pos, int32_t* n_eligible, ssw_gpu_result* results,
                                    uint32_t** cigar_pool, int64_t* cigar_words)
{
	const char* const who = "pool_align_windows_topk";
	if (!p) return -1;
	if (cigar_pool) *cigar_pool = 0;
	if (cigar_words) *cigar_words = 0;
	if (k < 1 || k > SSW_GPU_GROUP_TOPK_MAX) { snprintf(p->err, sizeof p->err, "%s: k must be 1 .. %d (k = %d)", who, SSW_GPU_GROUP_TOPK_MAX, k); return -1; }
	if (!qoffsets || nq < 0 || ngroups < 0 || !prm || !prm->mat || (ngroups > 0 && (!cand_off || !pos || !n_eligible || !results))) {
		snprintf(p->err, sizeof p->err, "%s: NULL argument", who);
		return -1;
	}
	if (!p->w[0].targets || !p->toff) { snprintf(p->err, sizeof p->err, "%s: no target set (ssw_gpu_pool_set_targets)", who); return -1; }
	if (ngroups > 0) {
		if (cand_off[0] != 0) { snprintf(p->err, sizeof p->err, "%s: cand_off[0] must be 0 (group 0 starts at candidate %lld)", who, (long long)cand_off[0]); return -1; }
		for (int64_t g = 0; g < ngroups; ++g)
			if (cand_off[g + 1] < cand_off[g]) {
				snprintf(p->err, sizeof p->err, "%s: cand_off decreases (group %lld: candidates [%lld, %lld))", who, (long long)g, (long long)cand_off[g],
				         (long long)cand_off[g + 1]);
				return -1;
			}
		const int64_t np = cand_off[ngroups];
		if (np > 0 && (!qidx || !tidx || !tbeg || !tlen)) { snprintf(p->err, sizeof p->err, "%s: NULL argument", who); return -1; }
		if (pool_windows_check(p, who, nq, with_revcomp, qidx, tidx, tbeg, tlen, np)) return -1;
	}
	pool_reset_stats(p);
	if (ngroups == 0) return 0;
	pool_call c; memset(&c, 0, sizeof c);
	c.qcodes = qcodes; c.qoff = qoffsets; c.nq = nq; c.prm = prm; c.results = results;
	c.cand_off = cand_off; c.wq = qidx; c.wt = tidx; c.wbeg = tbeg; c.wlen = tlen;
	c.wk = k; c.min_score = min_score; c.max_drop = max_drop; c.pos = pos; c.n_eligible = n_eligible;
	if (block <= 0) block = windows_auto_block(p, cand_off[ngroups]);
	c.nblocks = cut_groups(cand_off, ngroups, 1, block, 0);
	c.bstart = (int64_t*)malloc(sizeof(int64_t) * ((size_t)c.nblocks + 1));
	if (!c.bstart) { snprintf(p->err, sizeof p->err, "out of host memory (block list)"); return -1; }
	cut_groups(cand_off, ngroups, 1, block, c.bstart);
	c.nunits = ngroups; c.gpu = 1; c.width = k; c.run = run_windows; c.unit = "groups";
	const int rc = pool_run(p, &c, cigar_pool, cigar_words);
	free(c.bstart);
	return rc;
}

/* ssw_gpu_align_windows_mates_lib over the pool: a unit is a fragment -- two groups, two records, one selection.  Every check of the
   single-context call is made here over the whole list, so that the message names the caller's fragment, mate or pair and nothing is
   written before it */
static int pool_mates(ssw_gpu_pool* p, const char* who, const int8_t* qcodes, const int64_t* qoffsets, int32_t nq, int with_revcomp,
                      const int64_t* cand_off, int64_t nfrag,
                      const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                      int64_t block, const ssw_gpu_params* prm, int32_t min_score,
                      int32_t min_insert, int32_t max_insert, int32_t unpaired_penalty, int32_t orientation, const uint16_t* ins_pen,
                      ssw_gpu_mates* sel, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!qoffsets || nq < 0 || nfrag < 0 || !prm || !prm->mat || (nfrag > 0 && (!cand_off || !sel || !results))) {
		snprintf(p->err, sizeof p->err, "%s: NULL argument", who);
		return -1;
	}
	if (!p->w[0].targets || !p->toff) { snprintf(p->err, sizeof p->err, "%s: no target set (ssw_gpu_pool_set_targets)", who); return -1; }
	if (min_insert < 0 || min_insert > max_insert) {
		snprintf(p->err, sizeof p->err, "%s: 0 <= min_insert <= max_insert required (min_insert = %d, max_insert = %d)", who, min_insert, max_insert);
		return -1;
	}
	if (unpaired_penalty < 0 || unpaired_penalty > 65535) {
		snprintf(p->err, sizeof p->err, "%s: unpaired_penalty must be 0 .. 65535 (unpaired_penalty = %d)", who, unpaired_penalty);
		return -1;
	}
	if (orientation < SSW_GPU_MATES_FR || orientation > SSW_GPU_MATES_FF) {
		snprintf(p->err, sizeof p->err, "%s: orientation must be SSW_GPU_MATES_FR, _RF or _FF (orientation = %d)", who, orientation);
		return -1;
	}
	if (ins_pen && (int64_t)max_insert - min_insert + 1 > SSW_GPU_INSERT_TABLE_MAX) {
		snprintf(p->err, sizeof p->err, "%s: insert_penalty covers more than 65536 spans (min_insert = %d, max_insert = %d: %lld entries)", who, min_insert,
		         max_insert, (long long)max_insert - min_insert + 1);
		return -1;
	}
	if (nfrag > 0x7fffff00 / 2) {
		snprintf(p->err, sizeof p->err, "%s: more than 2^31 output slots in one call (%lld fragments)", who, (long long)nfrag);
		return -1;
	}
	if (nfrag > 0) {
		if (cand_off[0] != 0) {
			snprintf(p->err, sizeof p->err, "%s: cand_off[0] must be 0 (fragment 0 starts at candidate %lld)", who, (long long)cand_off[0]);
			return -1;
		}
		for (int64_t g = 0; g < 2 * nfrag; ++g) {
			const int64_t sz = cand_off[g + 1] - cand_off[g];
			if (sz >= 0 && sz <= SSW_GPU_MATES_GROUP_MAX) continue;
			snprintf(p->err, sizeof p->err, "%s: %s (fragment %lld, mate %d: candidates [%lld, %lld))", who,
			         sz < 0 ? "cand_off decreases" : "more than 4096 candidates in a group", (long long)(g >> 1), (int)(g & 1) + 1,
			         (long long)cand_off[g], (long long)cand_off[g + 1]);
			return -1;
		}
		const int64_t np = cand_off[2 * nfrag];
		if (np > 0 && (!qidx || !tidx || !tbeg || !tlen)) { snprintf(p->err, sizeof p->err, "%s: NULL argument", who); return -1; }
		if (pool_windows_check(p, who, nq, with_revcomp, qidx, tidx, tbeg, tlen, np)) return -1;
	}
	pool_reset_stats(p);
	if (nfrag == 0) return 0;
	pool_call c; memset(&c, 0, sizeof c);
	c.qcodes = qcodes; c.qoff = qoffsets; c.nq = nq; c.prm = prm; c.results = results;
	c.cand_off = cand_off; c.wq = qidx; c.wt = tidx; c.wbeg = tbeg; c.wlen = tlen;
	c.min_score = min_score; c.mates = sel;
	c.min_insert = min_insert; c.max_insert = max_insert; c.unpaired_penalty = unpaired_penalty; c.orientation = orientation;
	c.ins_pen = ins_pen;
	if (block <= 0) block = windows_auto_block(p, cand_off[2 * nfrag]);
	c.nblocks = cut_groups(cand_off, nfrag, 2, block, 0);
	c.bstart = (int64_t*)malloc(sizeof(int64_t) * ((size_t)c.nblocks + 1));
	if (!c.bstart) { snprintf(p->err, sizeof p->err, "out of host memory (block list)"); return -1; }
	cut_groups(cand_off, nfrag, 2, block, c.bstart);
	c.nunits = nfrag; c.gpu = 2; c.width = 2; c.run = run_windows; c.unit = "fragments";
	const int rc = pool_run(p, &c, cigar_pool, cigar_words);
	free(c.bstart);
	return rc;
}

int ssw_gpu_pool_align_windows_mates(ssw_gpu_pool* p, const int8_t* qcodes, const int64_t* qoffsets, int32_t nq, int with_revcomp,
                                     const int64_t* cand_off, int64_t nfrag,
                                     const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                                     int64_t block, const ssw_gpu_params* prm, int32_t min_score,
                                     int32_t min_insert, int32_t max_insert, int32_t unpaired_penalty, int32_t orientation,
                                     ssw_gpu_mates* sel, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!p) return -1;
	if (cigar_pool) *cigar_pool = 0;
	if (cigar_words) *cigar_words = 0;
	return pool_mates(p, "pool_align_windows_mates", qcodes, qoffsets, nq, with_revcomp, cand_off, nfrag, qidx, tidx, tbeg, tlen, block, prm, min_score,
	                  min_insert, max_insert, unpaired_penalty, orientation, 0, sel, results, cigar_pool, cigar_words);
}

/* ssw_gpu_align_windows_mates_model over the pool: the same blocks and checks, the model's table handed to every worker's call */
int ssw_gpu_pool_align_windows_mates_model(ssw_gpu_pool* p, const int8_t* qcodes, const int64_t* qoffsets, int32_t nq, int with_revcomp,
                                           const int64_t* cand_off, int64_t nfrag,
                                           const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                                           int64_t block, const ssw_gpu_params* prm, int32_t min_score, const ssw_gpu_pair_model* model,
                                           ssw_gpu_mates* sel, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!p) return -1;
	if (cigar_pool) *cigar_pool = 0;
	if (cigar_words) *cigar_words = 0;
	if (!model) { snprintf(p->err, sizeof p->err, "pool_align_windows_mates_model: NULL argument (model)"); return -1; }
	return pool_mates(p, "pool_align_windows_mates_model", qcodes, qoffsets, nq, with_revcomp, cand_off, nfrag, qidx, tidx, tbeg, tlen, block, prm,
	                  min_score, model->min_insert, model->max_insert, model->unpaired_penalty, model->orientation, model->insert_penalty, sel, results,
	                  cigar_pool, cigar_words);
}

static int pool_run(ssw_gpu_pool* p, pool_call* kk, uint32_t** cigar_pool, int64_t* cigar_words)
{
	pool_call k = *kk;
	ssw_gpu_result* results = k.results;
	k.pool = p;
	if (!k.bstart) k.nblocks = (k.nunits + k.block - 1) / k.block;
	k.want_cigars = cigar_pool != 0;
	k.cig = (block_cigars*)calloc((size_t)k.nblocks, sizeof(block_cigars));
	pthread_t* th = (pthread_t*)malloc(sizeof(pthread_t) * (size_t)p->n);
	pool_thread_arg* ta = (pool_thread_arg*)malloc(sizeof(pool_thread_arg) * (size_t)p->n);
	if (!k.cig || !th || !ta) { free(k.cig); free(th); free(ta); snprintf(p->err, sizeof p->err, "out of host memory"); return -1; }
	pthread_mutex_init(&k.err_lock, 0);
	int started = 0;
	for (int i = 0; i < p->n; ++i) {
		ta[i].call = &k; ta[i].widx = i;
		if (pthread_create(&th[i], 0, pool_thread, &ta[i])) break;
		++started;
	}
	if (started == 0) { __atomic_store_n(&k.failed, 1, __ATOMIC_RELEASE); snprintf(p->err, sizeof p->err, "pthread_create failed"); }
	for (int i = 0; i < started; ++i) pthread_join(th[i], 0);      /* (fewer threads than workers still drain the whole queue) */
	pthread_mutex_destroy(&k.err_lock);
	int rc = k.failed ? -1 : 0;
	if (rc == 0 && k.want_cigars) {   /* one pool in block order; a record's cigar_off was relative to its block's pool */
		int64_t total = 0;
		for (int64_t b = 0; b < k.nblocks; ++b) total += k.cig[b].n;
		uint32_t* all = total > 0 ? (uint32_t*)malloc(sizeof(uint32_t) * (size_t)total) : 0;
		if (total > 0 && !all) { snprintf(p->err, sizeof p->err, "out of host memory (CIGAR pool)"); rc = -1; }
		else {
			int64_t base = 0;
			for (int64_t b = 0; b < k.nblocks; ++b) {
				if (k.cig[b].n > 0) {
					memcpy(all + base, k.cig[b].words, sizeof(uint32_t) * (size_t)k.cig[b].n);
					int64_t u0, cnt;
					block_range(&k, b, &u0, &cnt);
					ssw_gpu_result* r = results + u0 * k.width;
					if (base > 0) for (int64_t i = 0; i < cnt * k.width; ++i) if (r[i].cigar_off >= 0) r[i].cigar_off += base;
				}
				base += k.cig[b].n;
			}
			*cigar_pool = all;
			if (cigar_words) *cigar_words = total;
		}
	}
	for (int64_t b = 0; b < k.nblocks; ++b) free(k.cig[b].words);
	free(k.cig); free(th); free(ta);
	return rc;
}
