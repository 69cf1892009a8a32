/*
 * ssw_host.c -- C host driver of the MI355X-native Smith-Waterman library.
 *
 * Implements the ssw.h ABI (ssw_init / ssw_align / init_destroy / align_destroy, replacing reference
 * src/ssw.c:826-982) and the batch ABI of ssw_gpu.h on top of the HIP kernels, reached only through
 * the thin shim declared in ssw_dev.h.  There is no CPU implementation of the alignment in this
 * library: without a device, or for parameters the kernels do not cover, calls fail loudly.
 *
 * Batch pipeline per target (one HIP stream; the database search and the traceback rounds fan out over side streams):
 *   queries bucketed by chain geometry and paired
 *     short (<= 384):  k_fill<R> (column maxima + 16-column group maxima of every tile)  ->  k_reduce_seg
 *     long:            k_chainq<R> (row strips drawn from a work queue, best cell tracked)  ->  k_reduce
 *     database search (flag 0, several short targets): k_filldb<R>, size classes side by side, records final
 *   -> [flag != 0] window passes (k_capture<R> / k_chainq<R, window>): read_end1 where not tracked, then the begin position
 *   -> [CIGAR wanted] k_trace / k_trace_wave rounds with negotiated scratch  -> [SAM] k_mark  -> records + CIGAR pool to the host.
 * ssw_gpu_search_db streams the database search chunk by chunk; csrc/ssw_pool.c spreads batches over several devices.
 */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <pthread.h>
#include "ssw.h"
#include "ssw_gpu.h"
#ifdef SSW_GPU_TEST_HOOKS
#include "ssw_gpu_diag.h"      /* the diagnostics exist in the test-hooks build only */
#endif
#include "ssw_dev.h"

_Static_assert(sizeof(struct ssw_out_rec) == sizeof(ssw_gpu_result), "device record layout must equal ssw_gpu_result");
_Static_assert(sizeof(struct ssw_mate_rec) == sizeof(ssw_gpu_mates) && sizeof(ssw_gpu_mates) == 32, "device selection layout must equal ssw_gpu_mates");
_Static_assert(sizeof(struct ssw_rescue_slot) == sizeof(ssw_gpu_rescued) && sizeof(ssw_gpu_rescued) == 24, "device rescue slot layout must equal ssw_gpu_rescued");
_Static_assert(SSW_MATES_GROUP_MAX == SSW_GPU_MATES_GROUP_MAX, "the kernel's group limit is the header's");
_Static_assert(SSW_MATES_FR == SSW_GPU_MATES_FR && SSW_MATES_RF == SSW_GPU_MATES_RF && SSW_MATES_FF == SSW_GPU_MATES_FF, "the kernel's orientations are the header's");
_Static_assert(sizeof(struct ssw_best_rec) == sizeof(ssw_gpu_best) && sizeof(ssw_gpu_best) == 16, "device record layout must equal ssw_gpu_best");

struct _profile {
	const int8_t* read;    /* borrowed, like the reference (src/ssw.c:842-843) */
	const int8_t* mat;     /* borrowed */
	int32_t readLen;
	int32_t n;
	int8_t score_size;
};

typedef struct { void* p; size_t cap; } dbuf;

/* Test / experiment hooks (SSW_GPU_* environment variables).  They are read ONCE at the entry of a batch call (knobs_load) into this
   record -- never inside the launch loops -- so that a test can flip one between two calls on the same context. */
typedef struct {
	int debug;              /* SSW_GPU_DEBUG: progress lines on stderr (and a stream sync after the queue launches) */
	int frame_k;            /* SSW_GPU_FRAME_K >= 16: renormalisation period of the column frame (tests: renormalise often); 0: default */
	int queue_mode;         /* SSW_GPU_QUEUE=jobs -> 1, strips -> 2, else 0: by the number of jobs */
	int queue_waves;        /* SSW_GPU_QUEUE_WAVES: wavefronts of a persistent launch; 0: what the device holds */
	int db_plain;           /* SSW_GPU_DB_FORM=0: k_filldb in the plain int16 form */
	int db_chain_best;      /* SSW_GPU_DB_CHAIN_BEST=0 switches the chain-best filter off */
	int xlanes16;           /* SSW_GPU_XLANES=16: long queries on 16-lane chains (k_chainx) */
	int xr, xr_window;      /* SSW_GPU_XR / SSW_GPU_XR_WINDOW: rows per lane of the strip kernel / of its window passes; 0: default */
	int fill_plain;         /* SSW_GPU_FILL_FORM=0 (or the older SSW_GPU_FILL_F16=0): plain int16 form everywhere */
	int no_db;              /* SSW_GPU_NO_DB=1: never take the fused database-search path */
	int overlap;            /* SSW_GPU_OVERLAP=1: reductions on a second stream beside the next fill (measured slower) */
	int no_track;           /* SSW_GPU_NO_TRACK=1: always run the locate pass */
	int no_seg_reduce;      /* SSW_GPU_SEG_REDUCE=0: k_reduce over the columns instead of k_reduce_seg over group maxima */
	int window_int16;       /* SSW_GPU_WINDOW_INT16: window passes of the strip kernel in the plain form */
	int trace_wave;         /* SSW_GPU_TRACE_WAVE=0/1: force the thread / team traceback; -1: by read length */
	int trace_no_lds;       /* SSW_GPU_TRACE_LDS=0: band rows in HBM scratch */
	int trace_waves;        /* SSW_GPU_TRACE_WAVES=1/4/16: team size; 0: by band width */
	int trace_unblocked;    /* SSW_GPU_TRACE_BLOCKED=0: teams with one cell per thread */
	int trace_many;         /* SSW_GPU_TRACE_MANY=<n>: a traceback round with more than n pending alignments sizes its teams for throughput (tests: 0); default 4096 */
	int trace_early;        /* SSW_GPU_TRACE_EARLY=<n>: batches of at least n tracebacks start the teams of the alignments that are wide from the start beside round 0.  Built and measured in
	                           round 6: SLOWER (config 4's traceback 175 -> 221 ms), off by default (0 / unset: never) -- kept with its tests as the measured form of "overlap the tail" */
	int trace_w1max, trace_w4max, trace_headroom;      /* SSW_GPU_TRACE_W1MAX / _W4MAX / _HEADROOM: widest doubled band (2b) walked by a one- / four-wavefront team when a round is about latency (96 / 256), scratch granted as a multiple of what the band that did not fit wants (8) */
	int pipe_any_count;     /* SSW_GPU_PIPE_EVEN=0: a pipelined series may have a number of launches that the streams do not share evenly (the form before this was measured) */
	int pipe_low_prio;      /* SSW_GPU_PIPE_PRIO=low: the extra streams of a pipelined series at the LOWEST dispatch priority (the first form of round 6; measured slower) */
	int pipe_parts;         /* SSW_GPU_PIPE_PARTS=2..8: the number of scratch parts / streams of a pipelined series (default 2; more were measured slower) */
	int no_fill_half;       /* SSW_GPU_FILL_HALF=0: the 16-lane kernel also where the half-row chains (k_fill8) apply */
	int no_fill_pairs;      /* SSW_GPU_FILL_PAIRS=0: k_fill8's diagonal-gap form with every plain add on its own (fill args dg = 2: the form before the adds went in pairs) */
	int no_fill_dg;         /* SSW_GPU_FILL_DG=0: k_fill8 opens gaps from every H (the recurrence before the diagonal-gap form) also where the scoring allows the diagonal alone */
	int no_pipe;            /* SSW_GPU_PIPE=0: the launches of a chunked short-query bucket one after the other on the main stream (the form before round 6) */
	int no_lit_spec;        /* SSW_GPU_LIT_SPEC=0: the lane-model kernel runs its 16-bit rules after the 8-bit ones (never both side by side: the form before round 6) */
	int trace_no_cls80;     /* SSW_GPU_TRACE_CLS80=0: no 80-KiB LDS class for the traceback teams (the classes before round 6) */
	int trace_diag;         /* SSW_GPU_TRACE_DIAG=1: the anti-diagonal narrow-band kernel (k_trace_diag, four alignments per wavefront) in front of the row
	                           kernels.  Built, bit-exact, measured in round 5 and NOT faster (52.8 ms against ~48 ms of the row kernel for the same 10^4
	                           alignments of config 4): kept for tests and as a starting point, off by default */
	int serial_buckets;     /* SSW_GPU_SERIAL_BUCKETS=1: geometry buckets one after the other on the main stream (the form before round 4) */
	int no_dbx;             /* SSW_GPU_NO_DBX=1: flagged batches against many targets take the per-target loop (the form before round 4) */
	int no_tail;            /* SSW_GPU_NO_TAIL=1: equal strips for long queries (no short last strip of the strip kernel: the form before the end of round 4) */
	int no_band;            /* SSW_GPU_NO_BAND=1: the capped reverse pass of the strip kernel visits whole windows (the form before round 4) */
	int call_trace;         /* SSW_GPU_CALL_TRACE=1: host timestamps of the phases of every batch call on stderr */
	int istat_groups;       /* SSW_GPU_ISTAT_GROUPS=<n>: k_insertstat on a grid of n workgroups, never more than the fragments need (tests: n = 1, 2 make a few dozen fragments cross the stride loop); 0: four per compute unit */
	int db_tsub, dbx_slab;  /* SSW_GPU_DB_TSUB / SSW_GPU_DBX_SLAB: targets per chunk of the database search / survivors per traceback slab (tests: force
	                           several chunks and slabs on toy batches); 0: from the budget */
} ssw_knobs;

#define SSW_TSTREAMS 6
#define SSW_PSTREAMS 7     /* extra streams of a pipelined series: up to 8 parts (SSW_GPU_PIPE_PARTS) */
#define DB_STREAMS 4                   /* side streams the size classes of a database-search chunk are spread over */

struct ssw_gpu_ctx {
	int device;
	void* stream;
	void* stream2;                      /* reductions of chunk i overlap the fill of chunk i+1 */
	void* pstream[SSW_PSTREAMS]; void* ev_pipe[SSW_PSTREAMS]; /* launches 1, 2, .. (mod the number of parts) of a pipelined series of fills (align_batch "pipe"), created with the first series that needs them */
	void* ustream;                      /* sequence uploads / translation (ssw_gpu_seqs_*): beside a running batch call, see upload_stream() */
	void* tstream[SSW_TSTREAMS]; void* tev[SSW_TSTREAMS];   /* traceback classes of one negotiation round run side by side */
	void *ev_fill[2], *ev_red[2];
	char err[512];
	pthread_mutex_t mu;                 /* guards the lazily created streams and the error text: ONE other thread may upload sequences while a batch call runs */
	ssw_gpu_timing tm;
	dbuf mat, pairs, pairs2, qlist, res, cm16, cm8, cm16b, cm8b, scratch, cigar, cigar2, need, goff, gpool, bnd, tlist, cand, tresume, queue, cands, sg16, sg8, qerr, fmtab, wtab, brec, bmap, dbjobs;
	dbuf sres, svq, svt, scnt;          /* flagged database search: survivor records, their (query, target) maps, counters */
	dbuf scratch0, need0, list0;        /* traceback: round 0 of the narrow alignments while the wide ones' teams already run (trace_phase "early") */
	dbuf tk_hits0, tk_hits1, tk_lst;    /* top-K search: the two chunk record buffers, the per-query lists + their state */
	void** ev; int nev, capev;          /* event pairs around fill launches */
	void *ev_t0, *ev_a, *ev_b, *ev_c, *ev_d, *ev_db;
	size_t cm_budget;                   /* bytes allowed for the two column-max buffers */
	int busy;                           /* a batch call is running on this context (one call at a time per context) */
	int side_ready;                     /* the side streams exist (ctx_side_streams) */
	int budget_shrunk;                  /* an allocation failed once: the device is shared, the budget was cut (plan_retreat) */
	ssw_knobs kn;                       /* environment hooks of the running call (knobs_load) */
	int dev_cus, dev_wave_slots;        /* compute units and resident wavefront slots of the device (hipGetDeviceProperties) */
	int device_share;                   /* > 1: that many single-pair calls of this process are in flight right now (ssw_align): a small call sizes its tiles for its share of the device */
	int queue_used;                     /* a work-queue launch of this call may have raised the error word (c->qerr): checked before results are handed out */
	void* hits_d[2]; void* hits_h[2]; size_t hits_cap;     /* streamed database search: two device + two page-locked host buffers, kept between calls */
};

struct ssw_gpu_seqs {
	ssw_gpu_ctx* ctx;
	int8_t* d_codes;
	int64_t* d_off;
	int64_t* h_off;
	int32_t count;
	int64_t total;
	/* every residue code of the set lies in [code_lo, code_hi] (codes_ranged; 0: not known).  The fill kernels turn a code outside [0, n) into a
	   null column; k_fill8's diagonal-gap form is exact only for targets without one (fill8_diag_gaps) */
	int codes_ranged; int32_t code_lo, code_hi;
};

static __thread char g_open_err[512];   /* error of the last failed ssw_gpu_open of this thread */

/* SSW_GPU_CALL_TRACE=1: host wall-clock at the phases of a batch call (what a single-pair ssw_align spends where) */
#define CALL_TRACE(what) do { if (c->kn.call_trace) fprintf(stderr, "[ssw_gpu call] %9.3f ms  %s\n", dbg_ms(), what); } while (0)

#ifdef SSW_GPU_TEST_HOOKS
static int env_int(const char* name, int dflt) { const char* e = getenv(name); return e && e[0] ? atoi(e) : dflt; }
#endif
static int env_is(const char* name, char ch) { const char* e = getenv(name); return e && e[0] == ch; }
/* The PRODUCT library (libssw.so) reads two diagnostics here -- SSW_GPU_DEBUG, SSW_GPU_CALL_TRACE -- and nothing that changes which kernel
   form runs: the form-switching hooks below exist only in the build the test suite and the measurement scripts load
   (-DSSW_GPU_TEST_HOOKS: libssw_hooks.so, tests/emu/libssw_emu.so; same host source, and the same kernels source with the few instantiations
   that only a hook selects -- libssw_hooks.so links a kernels object of its own for them). */
static void knobs_load(ssw_knobs* k)
{
	memset(k, 0, sizeof *k);
	k->debug = getenv("SSW_GPU_DEBUG") != 0;
	k->call_trace = env_is("SSW_GPU_CALL_TRACE", '1');
	k->db_chain_best = 1;
	k->trace_wave = -1;
	k->trace_many = 4096;
	k->trace_w1max = 96; k->trace_w4max = 256; k->trace_headroom = 8;
#ifdef SSW_GPU_TEST_HOOKS
	{ const int v = env_int("SSW_GPU_FRAME_K", 0); k->frame_k = v >= 16 ? v : 0; }
	k->queue_mode = env_is("SSW_GPU_QUEUE", 'j') ? 1 : env_is("SSW_GPU_QUEUE", 's') ? 2 : 0;
	{ const int v = env_int("SSW_GPU_QUEUE_WAVES", 0); k->queue_waves = v > 0 ? v : 0; }
	k->db_plain = env_is("SSW_GPU_DB_FORM", '0');
	k->db_chain_best = !env_is("SSW_GPU_DB_CHAIN_BEST", '0');
	k->xlanes16 = env_int("SSW_GPU_XLANES", 0) == 16;
	{ const int v = env_int("SSW_GPU_XR", 0); k->xr = v >= 1 && v <= 16 ? v : 0; }
	{ const int v = env_int("SSW_GPU_XR_WINDOW", 0); k->xr_window = v >= 1 && v <= 16 ? v : 0; }
	k->fill_plain = env_is("SSW_GPU_FILL_FORM", '0') || env_is("SSW_GPU_FILL_F16", '0');
	k->no_db = env_is("SSW_GPU_NO_DB", '1');
	k->overlap = env_is("SSW_GPU_OVERLAP", '1');
	k->no_track = env_is("SSW_GPU_NO_TRACK", '1');
	k->no_seg_reduce = env_is("SSW_GPU_SEG_REDUCE", '0');
	k->window_int16 = getenv("SSW_GPU_WINDOW_INT16") != 0;
	k->trace_wave = getenv("SSW_GPU_TRACE_WAVE") ? env_is("SSW_GPU_TRACE_WAVE", '1') : -1;
	k->trace_no_lds = env_is("SSW_GPU_TRACE_LDS", '0');
	{ const int v = env_int("SSW_GPU_TRACE_WAVES", 0); k->trace_waves = v == 1 || v == 4 || v == 16 ? v : 0; }
	k->trace_unblocked = env_is("SSW_GPU_TRACE_BLOCKED", '0');
	k->trace_diag = env_is("SSW_GPU_TRACE_DIAG", '1');
	if (getenv("SSW_GPU_TRACE_MANY")) k->trace_many = env_int("SSW_GPU_TRACE_MANY", 4096);
	k->serial_buckets = env_is("SSW_GPU_SERIAL_BUCKETS", '1');
	k->no_dbx = env_is("SSW_GPU_NO_DBX", '1');
	k->no_band = env_is("SSW_GPU_NO_BAND", '1');
	k->trace_no_cls80 = env_is("SSW_GPU_TRACE_CLS80", '0');
	k->no_lit_spec = env_is("SSW_GPU_LIT_SPEC", '0');
	k->no_pipe = env_is("SSW_GPU_PIPE", '0');
	k->no_fill_half = env_is("SSW_GPU_FILL_HALF", '0');
	k->no_fill_dg = env_is("SSW_GPU_FILL_DG", '0');
	k->no_fill_pairs = env_is("SSW_GPU_FILL_PAIRS", '0');
	k->pipe_low_prio = env_is("SSW_GPU_PIPE_PRIO", 'l');
	k->pipe_any_count = env_is("SSW_GPU_PIPE_EVEN", '0');
	{ const int v = env_int("SSW_GPU_TRACE_W1MAX", 0); if (v >= 2 && v <= 254) k->trace_w1max = v; }
	{ const int v = env_int("SSW_GPU_TRACE_W4MAX", 0); if (v >= 2 && v <= 3070) k->trace_w4max = v; }
	{ const int v = env_int("SSW_GPU_TRACE_HEADROOM", 0); if (v >= 2 && v <= 64) k->trace_headroom = v; }
	{ const int v = env_int("SSW_GPU_PIPE_PARTS", 0); k->pipe_parts = v >= 2 && v <= 8 ? v : 0; }
	k->trace_early = env_int("SSW_GPU_TRACE_EARLY", 0);
	k->no_tail = env_is("SSW_GPU_NO_TAIL", '1');
	{ const int v = env_int("SSW_GPU_DB_TSUB", 0); k->db_tsub = v > 0 ? v : 0; }
	{ const int v = env_int("SSW_GPU_DBX_SLAB", 0); k->dbx_slab = v > 0 ? v : 0; }
	{ const int v = env_int("SSW_GPU_ISTAT_GROUPS", 0); k->istat_groups = v > 0 ? v : 0; }
#endif
}
#ifdef SSW_GPU_TEST_HOOKS
/* this build reads the form-switching SSW_GPU_* hooks (tests refuse to run their variants on a library that would ignore them; libssw.so has
   no such symbol: include/ssw_gpu_diag.h) */
int ssw_gpu_has_test_hooks(void) { return 1; }
#endif

#include <time.h>
static double dbg_ms(void)      /* wall clock for the SSW_GPU_DEBUG progress lines */
{
	struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t);
	return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

static int fail(ssw_gpu_ctx* c, const char* fmt, const char* detail)
{
	if (!c) { snprintf(g_open_err, 512, fmt, detail ? detail : ""); return -1; }
	char tmp[512];
	snprintf(tmp, sizeof tmp, fmt, detail ? detail : "");
	pthread_mutex_lock(&c->mu);      /* (a feeder thread's upload and the batch call may both fail: whole messages, one after the other) */
	memcpy(c->err, tmp, sizeof tmp);
	pthread_mutex_unlock(&c->mu);
	return -1;
}

static void* ensure(ssw_gpu_ctx* c, dbuf* b, size_t bytes)
{
	if (b->cap >= bytes && b->p) return b->p;
	if (b->p) { ssw_shim_stream_sync(c->stream); ssw_shim_free(b->p); b->p = 0; b->cap = 0; }
	size_t want = bytes + bytes / 8 + 256;
	b->p = ssw_shim_malloc(want);
	if (!b->p) { fail(c, "device allocation failed: %s", ssw_shim_last_error()); return 0; }
	b->cap = want;
	return b->p;
}

static void dbuf_free(dbuf* b) { if (b->p) ssw_shim_free(b->p); b->p = 0; b->cap = 0; }

int ssw_gpu_device_count(void) { return ssw_shim_device_count(); }

const char* ssw_gpu_last_error(const ssw_gpu_ctx* ctx) { return ctx ? ctx->err : g_open_err; }

ssw_gpu_ctx* ssw_gpu_open(int device)
{
	int n = ssw_shim_device_count();
	if (n <= 0) { fail(0, "no HIP device available (%s); this library has no CPU path", ssw_shim_last_error()); return 0; }
	if (device < 0 || device >= n) { fail(0, "device index out of range%s", ""); return 0; }
	if (ssw_shim_set_device(device)) { fail(0, "hipSetDevice failed: %s", ssw_shim_last_error()); return 0; }
	ssw_gpu_ctx* c = (ssw_gpu_ctx*)calloc(1, sizeof(*c));
	if (!c) { fail(0, "out of host memory%s", ""); return 0; }
	c->device = device;
	pthread_mutex_init(&c->mu, 0);
	c->stream = ssw_shim_stream_create();
	int ok = c->stream != 0;      /* (the side streams come with the first call that is more than one pair: ctx_side_streams) */
	for (int i = 0; i < 2; ++i) { c->ev_fill[i] = ssw_shim_event_create(); c->ev_red[i] = ssw_shim_event_create(); ok = ok && c->ev_fill[i] && c->ev_red[i]; }
	c->ev_t0 = ssw_shim_event_create(); c->ev_a = ssw_shim_event_create(); c->ev_b = ssw_shim_event_create();
	c->ev_c = ssw_shim_event_create(); c->ev_d = ssw_shim_event_create(); c->ev_db = ssw_shim_event_create();
	if (!ok || !c->ev_t0 || !c->ev_a || !c->ev_b || !c->ev_c || !c->ev_d || !c->ev_db) {
		fail(0, "stream/event creation failed: %s", ssw_shim_last_error());
		ssw_gpu_close(c);      /* destroys whatever was created (NULL handles are skipped) */
		return 0;
	}
	knobs_load(&c->kn);
	/* geometry of the device the launches are sized for: a partitioned (CPX / DPX) MI355X reports fewer compute units than the 256 of
	   the whole chip, and launches sized for 256 would leave its last round of workgroups half empty */
	c->dev_cus = 256; c->dev_wave_slots = 2048;
	{ int cus = 0, wpc = 0; if (ssw_shim_device_props(&cus, &wpc) == 0 && cus > 0) { c->dev_cus = cus; c->dev_wave_slots = cus * 8; } }
	const char* e = getenv("SSW_GPU_CM_BUDGET_MB");
	/* scratch budget (column maxima, boundary records, traceback scratch).  The DEFAULT assumes nothing about who else uses the device: half
	   of what is free now, at most 64 GiB -- several processes per GPU (ranks, single-pair callers) then still fit, and HIP does not refuse
	   an over-subscribing hipMalloc of another process: the failure would only show at a kernel launch.  A caller that has the device to
	   itself says so with ssw_gpu_set_budget_exclusive (bench.py does when every rank has its own GPU): 288 GB then hold 3 fill launches
	   per 100k reads of config 2 instead of 6. */
	c->cm_budget = e ? (size_t)atoll(e) << 20 : (size_t)64 << 30;
	if (!e) { size_t fr = ssw_shim_mem_free_bytes(); if (fr && c->cm_budget > fr / 2) c->cm_budget = fr / 2; }
	return c;
}

/* The side streams (reductions beside fills, buckets / size classes / traceback classes side by side) are created by the first call that can
   use them.  A context that only ever serves single-pair ssw_align calls keeps ONE stream: the runtime maps streams onto four hardware queues
   in creation order, and with eight streams per context the main streams of all caller threads' contexts landed on the SAME queue -- their
   calls ran one after the other however many threads called (scripts/probes/dropin_threads.c, profiles/round4_dropin_threads.txt). */
static int ctx_side_streams(ssw_gpu_ctx* c)
{
	/* under the context's lock (round-5 advisor): a feeder thread's FIRST upload creates these too (upload_stream), possibly while the first
	   batch call is on its way here -- created twice, the first set would leak and the hardware-queue order the launch plans assume change */
	pthread_mutex_lock(&c->mu);
	int ok = 1;
	if (!__atomic_load_n(&c->side_ready, __ATOMIC_ACQUIRE)) {
		c->stream2 = ssw_shim_stream_create();
		ok = c->stream2 != 0;
		for (int i = 0; i < SSW_TSTREAMS; ++i) { c->tstream[i] = ssw_shim_stream_create(); c->tev[i] = ssw_shim_event_create(); ok = ok && c->tstream[i] && c->tev[i]; }
		if (ok) __atomic_store_n(&c->side_ready, 1, __ATOMIC_RELEASE);
	}
	pthread_mutex_unlock(&c->mu);
	return ok ? 0 : fail(c, "stream/event creation failed: %s", ssw_shim_last_error());
}

/* Waits for everything a FAILED call may have left queued, on the main stream and on every side stream it can have launched to: its caller
   frees or reuses the buffers those launches read and write.  (Results ignored: the call reports its own error.) */
static void ctx_drain(ssw_gpu_ctx* c)
{
	ssw_shim_stream_sync(c->stream);
	if (__atomic_load_n(&c->side_ready, __ATOMIC_ACQUIRE)) {
		ssw_shim_stream_sync(c->stream2);
		for (int k = 0; k < SSW_TSTREAMS; ++k) ssw_shim_stream_sync(c->tstream[k]);
	}
	for (int k = 0; k < SSW_PSTREAMS; ++k) if (c->pstream[k]) ssw_shim_stream_sync(c->pstream[k]);
}

const char* ssw_gpu_strerror(int rc)
{
	switch (rc) {
	case 0: return "ok";
	case SSW_GPU_BUSY: return "the context is inside another call (one call at a time per context: open one context per thread)";
	case -1: return "the call failed: ssw_gpu_last_error(ctx) has the reason";
	default: return rc > 0 ? "stopped by the caller's chunk function (its return value)" : "the call failed";
	}
}

/* Column-maximum / scratch budget of this context in bytes (0: back to the default, min(64 GiB, half of the free HBM at the time of
   the call)).  Contexts that SHARE a device -- pool workers with repeated device indices, several ranks per GPU -- each take what
   they are given: ssw_gpu_pool_open divides the default by the workers on a device. */
int ssw_gpu_set_budget(ssw_gpu_ctx* c, size_t bytes)
{
	if (!c) return -1;
	if (__atomic_load_n(&c->busy, __ATOMIC_ACQUIRE)) return SSW_GPU_BUSY;
	if (bytes == 0) {
		ssw_shim_set_device(c->device);
		bytes = (size_t)64 << 30;
		size_t fr = ssw_shim_mem_free_bytes(); if (fr && bytes > fr / 2) bytes = fr / 2;
	}
	if (bytes < ((size_t)1 << 20)) bytes = (size_t)1 << 20;
	c->cm_budget = bytes;
	c->budget_shrunk = 0;      /* an explicit budget starts the allocation-retry ladder afresh */
	return 0;
}
size_t ssw_gpu_get_budget(const ssw_gpu_ctx* c) { return c ? c->cm_budget : 0; }

/* "This context has its device to itself": budget = min(200 GiB, 60 % of the free HBM).  Sized for the 288 GB of an MI355X. */
int ssw_gpu_set_budget_exclusive(ssw_gpu_ctx* c)
{
	if (!c) return -1;
	ssw_shim_set_device(c->device);
	size_t bytes = (size_t)200 << 30;
	const size_t fr = ssw_shim_mem_free_bytes();
	if (fr && bytes > fr / 5 * 3) bytes = fr / 5 * 3;
	return ssw_gpu_set_budget(c, bytes);
}

void ssw_gpu_close(ssw_gpu_ctx* c)
{
	if (!c) return;
	ssw_shim_set_device(c->device);
	if (c->stream) ssw_shim_stream_sync(c->stream);
	for (int i = 0; i < 2; ++i) { ssw_shim_free(c->hits_d[i]); ssw_shim_host_free(c->hits_h[i]); }
	dbuf_free(&c->mat); dbuf_free(&c->pairs); dbuf_free(&c->qlist); dbuf_free(&c->res); dbuf_free(&c->cm16);
	dbuf_free(&c->cm8); dbuf_free(&c->cm16b); dbuf_free(&c->cm8b); dbuf_free(&c->cigar2); dbuf_free(&c->scratch); dbuf_free(&c->cigar); dbuf_free(&c->need); dbuf_free(&c->goff); dbuf_free(&c->gpool); dbuf_free(&c->bnd); dbuf_free(&c->tlist); dbuf_free(&c->pairs2); dbuf_free(&c->cand); dbuf_free(&c->tresume); dbuf_free(&c->queue); dbuf_free(&c->cands); dbuf_free(&c->sg16); dbuf_free(&c->sg8); dbuf_free(&c->qerr); dbuf_free(&c->fmtab); dbuf_free(&c->wtab); dbuf_free(&c->brec); dbuf_free(&c->bmap); dbuf_free(&c->dbjobs);
	dbuf_free(&c->sres); dbuf_free(&c->svq); dbuf_free(&c->svt); dbuf_free(&c->scnt);
	dbuf_free(&c->scratch0); dbuf_free(&c->need0); dbuf_free(&c->list0);
	dbuf_free(&c->tk_hits0); dbuf_free(&c->tk_hits1); dbuf_free(&c->tk_lst);
	for (int i = 0; i < c->capev; ++i) ssw_shim_event_destroy(c->ev[i]);
	free(c->ev);
	ssw_shim_event_destroy(c->ev_t0); ssw_shim_event_destroy(c->ev_a); ssw_shim_event_destroy(c->ev_b);
	ssw_shim_event_destroy(c->ev_c); ssw_shim_event_destroy(c->ev_d); ssw_shim_event_destroy(c->ev_db);
	for (int i = 0; i < 2; ++i) { ssw_shim_event_destroy(c->ev_fill[i]); ssw_shim_event_destroy(c->ev_red[i]); }
	ssw_shim_stream_destroy(c->stream2); ssw_shim_stream_destroy(c->ustream); for (int i = 0; i < SSW_PSTREAMS; ++i) { ssw_shim_stream_destroy(c->pstream[i]); ssw_shim_event_destroy(c->ev_pipe[i]); }
	for (int i = 0; i < SSW_TSTREAMS; ++i) { ssw_shim_stream_destroy(c->tstream[i]); ssw_shim_event_destroy(c->tev[i]); }
	ssw_shim_stream_destroy(c->stream);
	pthread_mutex_destroy(&c->mu);
	free(c);
}

/* Sequence sets are uploaded (and translated / reverse-complemented) on a stream of their own, created with the first upload: ONE other
   thread may prepare the next block of reads on a context while a batch call runs on it (streaming callers: bench.py --config 3 --full,
   the three-stage ssw_test_gpu) and the copy does not queue behind that call's kernels.  Every ssw_gpu_seqs_* call returns with its stream
   synchronised, so a later batch call on the main stream sees the data.  (The single-pair path never gets here: its contexts keep one
   stream) */
static void* upload_stream(ssw_gpu_ctx* c)
{
	void* us = __atomic_load_n(&c->ustream, __ATOMIC_ACQUIRE);
	if (!us) {
		/* (after the side streams: the launch plans of a batch call know which hardware queue each of THOSE lands on by creation order) */
		(void)ctx_side_streams(c);
		pthread_mutex_lock(&c->mu);
		if (!c->ustream) __atomic_store_n(&c->ustream, ssw_shim_stream_create(), __ATOMIC_RELEASE);
		us = c->ustream;
		pthread_mutex_unlock(&c->mu);
	}
	return us ? us : c->stream;
}

/* host-side shell of a sequence set + its two device arrays (codes, offsets); NULL with the error set on failure */
static ssw_gpu_seqs* seqs_new(ssw_gpu_ctx* c, const int64_t* offsets, int32_t count)
{
	ssw_gpu_seqs* s = (ssw_gpu_seqs*)calloc(1, sizeof(*s));
	if (!s) { fail(c, "out of host memory%s", ""); return 0; }
	s->ctx = c; s->count = count; s->total = offsets[count] - offsets[0];
	s->h_off = (int64_t*)malloc(sizeof(int64_t) * ((size_t)count + 1));
	if (!s->h_off || s->total < 0) { fail(c, s->h_off ? "seqs: offsets must not decrease%s" : "out of host memory%s", ""); ssw_gpu_seqs_free(s); return 0; }
	for (int32_t i = 0; i <= count; ++i) s->h_off[i] = offsets[i] - offsets[0];
	for (int32_t i = 0; i < count; ++i) if (s->h_off[i + 1] < s->h_off[i]) { fail(c, "seqs: offsets must not decrease%s", ""); ssw_gpu_seqs_free(s); return 0; }
	s->d_codes = (int8_t*)ssw_shim_malloc((size_t)s->total + 64);   /* +64: ring prefetch may not run past the end, but keep slack */
	s->d_off = (int64_t*)ssw_shim_malloc(sizeof(int64_t) * ((size_t)count + 1));
	if (!s->d_codes || !s->d_off) { fail(c, "device allocation failed: %s", ssw_shim_last_error()); ssw_gpu_seqs_free(s); return 0; }
	return s;
}

ssw_gpu_seqs* ssw_gpu_seqs_upload(ssw_gpu_ctx* c, const int8_t* codes, const int64_t* offsets, int32_t count)
{
	if (!c || count < 0 || !offsets || (!codes && offsets[count] != offsets[0])) { fail(c, "seqs_upload: bad arguments%s", ""); return 0; }
	ssw_shim_set_device(c->device);
	ssw_gpu_seqs* s = seqs_new(c, offsets, count);
	if (!s) return 0;
	void* const us = upload_stream(c);
	if (ssw_shim_h2d(s->d_codes, codes + offsets[0], (size_t)s->total, us) ||
	    ssw_shim_h2d(s->d_off, s->h_off, sizeof(int64_t) * ((size_t)count + 1), us) ||
	    ssw_shim_stream_sync(us)) {
		fail(c, "upload failed: %s", ssw_shim_last_error()); ssw_gpu_seqs_free(s); return 0;
	}
	{
		const int8_t* p = codes + offsets[0];
		int lo = 127, hi = -128;
		for (int64_t i = 0; i < s->total; ++i) { if (p[i] < lo) lo = p[i]; if (p[i] > hi) hi = p[i]; }
		s->codes_ranged = 1; s->code_lo = lo; s->code_hi = hi;      /* (an empty set: lo > hi, inside every alphabet) */
	}
	return s;
}

void ssw_gpu_seqs_free(ssw_gpu_seqs* s)
{
	if (!s) return;
	if (s->ctx) ssw_shim_set_device(s->ctx->device);
	ssw_shim_free(s->d_codes); ssw_shim_free(s->d_off); free(s->h_off); free(s);
}

ssw_gpu_seqs* ssw_gpu_seqs_upload_ascii(ssw_gpu_ctx* c, const char* text, const int64_t* offsets, int32_t count, const int8_t* table128)
{
	if (!c || count < 0 || !offsets || !table128 || (!text && offsets[count] != offsets[0])) { fail(c, "seqs_upload_ascii: bad arguments%s", ""); return 0; }
	ssw_shim_set_device(c->device);
	ssw_gpu_seqs* s = seqs_new(c, offsets, count);
	if (!s) return 0;
	void* const us = upload_stream(c);
	uint8_t* d_text = (uint8_t*)ssw_shim_malloc((size_t)s->total + 64);
	int8_t* d_tab = (int8_t*)ssw_shim_malloc(128);
	int ok = d_text && d_tab;
	if (ok) {
		ssw_prep_args pa; memset(&pa, 0, sizeof pa);
		pa.text = d_text; pa.table = d_tab; pa.off = s->d_off; pa.count = count; pa.total = s->total; pa.out = s->d_codes; pa.mode = 0;
		ok = !(ssw_shim_h2d(d_text, text + offsets[0], (size_t)s->total, us) || ssw_shim_h2d(d_tab, table128, 128, us) ||
		       ssw_shim_h2d(s->d_off, s->h_off, sizeof(int64_t) * ((size_t)count + 1), us) ||
		       ssw_shim_launch_prep(&pa, us) || ssw_shim_stream_sync(us));
	}
	ssw_shim_free(d_text); ssw_shim_free(d_tab);
	if (!ok) { fail(c, "ascii upload failed: %s", ssw_shim_last_error()); ssw_gpu_seqs_free(s); return 0; }
	s->codes_ranged = 1; s->code_lo = 127; s->code_hi = -128;      /* whatever the table can deliver */
	for (int i = 0; i < 128; ++i) { if (table128[i] < s->code_lo) s->code_lo = table128[i]; if (table128[i] > s->code_hi) s->code_hi = table128[i]; }
	return s;
}

/* the complement maps the codes 0 .. 3 among themselves and leaves every other code as it is */
static void seqs_range_revcomp(ssw_gpu_seqs* s, const ssw_gpu_seqs* in)
{
	s->codes_ranged = in->codes_ranged;
	s->code_lo = in->code_lo < 0 || in->code_lo > in->code_hi ? in->code_lo : 0;
	s->code_hi = in->code_hi > 3 || in->code_lo > in->code_hi ? in->code_hi : 3;
}

ssw_gpu_seqs* ssw_gpu_seqs_revcomp(ssw_gpu_ctx* c, const ssw_gpu_seqs* in)
{
	if (!c || !in || in->ctx != c) { fail(c, "seqs_revcomp: bad arguments%s", ""); return 0; }
	ssw_shim_set_device(c->device);
	ssw_gpu_seqs* s = seqs_new(c, in->h_off, in->count);
	if (!s) return 0;
	void* const us = upload_stream(c);
	ssw_prep_args pa; memset(&pa, 0, sizeof pa);
	pa.codes_in = in->d_codes; pa.off = in->d_off; pa.count = in->count; pa.total = in->total; pa.out = s->d_codes; pa.mode = 1;
	if (ssw_shim_h2d(s->d_off, s->h_off, sizeof(int64_t) * ((size_t)in->count + 1), us) ||
	    ssw_shim_launch_prep(&pa, us) || ssw_shim_stream_sync(us)) {
		fail(c, "revcomp failed: %s", ssw_shim_last_error()); ssw_gpu_seqs_free(s); return 0;
	}
	seqs_range_revcomp(s, in);
	return s;
}

/* `in` (N sequences) followed by the reverse complement of every one of them: ONE set of 2 N sequences, sequence N + i = revcomp(sequence i).
   `ssw_test -r` aligns every read in both orientations (reference src/main.c:478-481, 507-519): with this set that is one batch call of
   2 N queries instead of two of N. */
ssw_gpu_seqs* ssw_gpu_seqs_with_revcomp(ssw_gpu_ctx* c, const ssw_gpu_seqs* in)
{
	if (!c || !in || in->ctx != c || in->count > 0x3fffffff) { fail(c, "seqs_with_revcomp: bad arguments%s", ""); return 0; }
	ssw_shim_set_device(c->device);
	const int32_t n = in->count;
	int64_t* off2 = (int64_t*)malloc(sizeof(int64_t) * (2 * (size_t)n + 1));
	if (!off2) { fail(c, "out of host memory%s", ""); return 0; }
	for (int32_t i = 0; i <= n; ++i) { off2[i] = in->h_off[i]; off2[n + i] = in->total + in->h_off[i]; }
	ssw_gpu_seqs* s = seqs_new(c, off2, 2 * n);
	free(off2);
	if (!s) return 0;
	void* const us = upload_stream(c);
	ssw_prep_args pa; memset(&pa, 0, sizeof pa);
	pa.codes_in = in->d_codes; pa.off = in->d_off; pa.count = n; pa.total = in->total; pa.out = s->d_codes; pa.mode = 2;
	if (ssw_shim_h2d(s->d_off, s->h_off, sizeof(int64_t) * (2 * (size_t)n + 1), us) ||
	    ssw_shim_launch_prep(&pa, us) || ssw_shim_stream_sync(us)) {
		fail(c, "revcomp failed: %s", ssw_shim_last_error()); ssw_gpu_seqs_free(s); return 0;
	}
	seqs_range_revcomp(s, in);
	return s;
}

/* copies the residue codes of a device-resident set back to the host (tests, debugging) */
int ssw_gpu_seqs_download(ssw_gpu_ctx* c, const ssw_gpu_seqs* s, int8_t* codes_out)
{
	if (!c || !s || !codes_out) return -1;
	ssw_shim_set_device(c->device);
	if (ssw_shim_d2h(codes_out, s->d_codes, (size_t)s->total, c->stream) || ssw_shim_stream_sync(c->stream)) return fail(c, "download failed: %s", ssw_shim_last_error());
	return 0;
}

int32_t ssw_gpu_seqs_count(const ssw_gpu_seqs* s) { return s ? s->count : 0; }

/* The timing record only ever grows at its END: a caller compiled against an older header passes its own sizeof and gets the
   fields it knows (ssw_gpu_last_timing_sized); ssw_gpu_last_timing is the current header's full record. */
int ssw_gpu_last_timing_sized(const ssw_gpu_ctx* c, void* out, size_t out_size)
{
	if (!c || !out) return -1;
	memcpy(out, &c->tm, out_size < sizeof c->tm ? out_size : sizeof c->tm);
	if (out_size > sizeof c->tm) memset((char*)out + sizeof c->tm, 0, out_size - sizeof c->tm);
	return 0;
}
int ssw_gpu_last_timing(const ssw_gpu_ctx* c, ssw_gpu_timing* out) { return ssw_gpu_last_timing_sized(c, out, sizeof *out); }

/* ------------------------------------------------------------------------------------------------ */

/* Column-frame form (lanes.h): stored values are true value + phi(column).  For gap penalties gapO > gapE and a bucket
   whose true scores stay <= top, picks the renormalisation period K (a power of two >= 64, K * gapE <= ~4096) and the base offset
   so that every live operand is a non-negative number below 0x7C00; returns 0 when the bucket does not fit (plain int16 form then).
   lanes = lanes per chain (16 or 64; 8: the half-row chains, whose blocked row frame holds the rows of class 3 a further 3 x gapE up). */
static int ssw_frame_params(const ssw_knobs* kn, int64_t top, int gapO, int gapE, int minmat, int lanes, int32_t* base, int32_t* kmask)
{
	if (gapO <= gapE || gapE < 1) return 0;
	int K = 1024;
	if (kn->frame_k) { K = 16; while (K * 2 <= kn->frame_k && K < 1024) K <<= 1; }   /* tests: renormalise often */
	while (K > 64 && (int64_t)K * gapE > 4096) K >>= 1;
	const int b = (minmat < 0 ? -minmat : 0) + gapO + 2 * gapE + 8;     /* diag + score' >= 0, F - gapE >= 0, t >= 0 */
	const int up = lanes + 2 + (lanes == 8 ? 3 : 0);
	/* a bucket near the top of the range still fits with a shorter period (15-kb reads at match 2, proteins with a large max(mat)): halve
	   K down to 64 before giving the bucket to the 9-instruction plain form */
	while (K > 64 && top + b + (int64_t)(K + up) * gapE >= 31744) K >>= 1;
	if (top + b + (int64_t)(K + up) * gapE >= 31744) return 0;
	*base = b; *kmask = K - 1;
	return 1;
}

/* k_fill8 may open gaps from the diagonal candidate alone (chain_row8<.., DG> in ssw_kernels.hip; DESIGN.md "Gaps from the diagonal"): that drops a
   vertical gap directly next to a horizontal one, which never scores more than the diagonal steps and the one gap that replace it when
   gapO > gapE and no entry of the matrix is below -2 gapE -- and when every cell of the rectangle has a diagonal, that is, the target has no
   null column: no residue code outside [0, n), known from the upload (a set whose range is not known keeps the full recurrence).  R8 = 9 and
   R8 = 17 have no instance of the form (RowFrame8<R>::DG in ssw_kernels.hip: no pairs / a wavefront per SIMD lost).  The frame needs nothing more: x - (gapO - gapE) of a live row is
   >= fr_base + gapE + min(mat) - (gapO - gapE) = 4 gapE + 8, and a dead half keeps H of the row above, >= fr_base + gapE, in its low 15 bits */
static int fill8_diag_gaps(const ssw_knobs* kn, const ssw_gpu_seqs* T, int R8, int32_t n, int32_t minmat, int gapO, int gapE)
{
	if (kn->no_fill_dg || R8 == 9 || R8 == 17 || gapO <= gapE) return 0;
	if (-(int64_t)minmat > 2 * (int64_t)gapE) return 0;
	return T->codes_ranged && (T->code_lo > T->code_hi || (T->code_lo >= 0 && T->code_hi < n));
}

static int32_t halo_for(int32_t P, int32_t maxmat, int32_t gapE)
{
	if (gapE <= 0) return 0x3fffffff;
	int64_t w = (int64_t)P + ((int64_t)P * (maxmat > 0 ? maxmat : 0) + gapE - 1) / gapE + 1;
	return w > 0x3fffffff ? 0x3fffffff : (int32_t)w;
}

static void* next_event(ssw_gpu_ctx* c)
{
	if (c->nev == c->capev) {
		int nc = c->capev ? c->capev * 2 : 64;
		void** ne = (void**)realloc(c->ev, sizeof(void*) * nc);
		if (!ne) return 0;     /* no memory for another timing event: this launch goes untimed (a NULL event is refused by the runtime) */
		c->ev = ne;
		for (int i = c->capev; i < nc; ++i) c->ev[i] = ssw_shim_event_create();
		c->capev = nc;
	}
	return c->ev[c->nev++];
}

/* ---- what every batch entry point shares ---- */

/* The context's streams, events and workspaces serve one call at a time (include/ssw_gpu.h "Threads").  SSW_GPU_BUSY: another thread is
   inside this context -- its error text is the running call's and is left alone (ssw_gpu_strerror names the code); the pool outputs of
   the refused call read as empty. */
static int ctx_enter(ssw_gpu_ctx* c, uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!__atomic_exchange_n(&c->busy, 1, __ATOMIC_ACQUIRE)) return 0;
	if (cigar_pool) *cigar_pool = 0;
	if (cigar_words) *cigar_words = 0;
	return SSW_GPU_BUSY;
}
static int ctx_leave(ssw_gpu_ctx* c, int rc) { __atomic_store_n(&c->busy, 0, __ATOMIC_RELEASE); return rc; }

static int fail_who(ssw_gpu_ctx* c, const char* who, const char* what)
{
	char msg[160];
	snprintf(msg, sizeof msg, "%s: %s", who, what);
	return fail(c, "%s", msg);
}
/* The argument checks of the batch entry points, in the order they fire: NULL arguments (an entry point checks its own further pointers
   first, with the same text), sequences of another context -- check_seqs --, then the alphabet size and score_size -- check_scoring.
   Only align_batch has a check of its own in between (its target range). */
static int check_seqs(ssw_gpu_ctx* c, const char* who, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const ssw_gpu_params* prm)
{
	if (!Q || !T || !prm || !prm->mat) return fail_who(c, who, "NULL argument");
	if (Q->ctx != c || T->ctx != c) return fail_who(c, who, "sequences belong to another context");
	return 0;
}
static int check_scoring(ssw_gpu_ctx* c, const char* who, const ssw_gpu_params* prm)
{
	if (prm->n < 1) return fail_who(c, who, "alphabet size must be >= 1");
	if (prm->score_size < 0 || prm->score_size > 2) return fail_who(c, who, "score_size must be 0, 1 or 2");
	return 0;
}
static int check_common(ssw_gpu_ctx* c, const char* who, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const ssw_gpu_params* prm)
{
	return check_seqs(c, who, Q, T, prm) || check_scoring(c, who, prm) ? -1 : 0;
}

/* smallest (<= 0) and largest (>= 0) entry of the WHOLE scoring matrix, and the 8-bit bias as ssw_init computes it (src/ssw.c:834-836) */
static void mat_range(const ssw_gpu_params* prm, int32_t* minmat, int32_t* maxmat, int32_t* bias)
{
	int32_t lo = 0, hi = 0;
	for (int64_t i = 0; i < (int64_t)prm->n * prm->n; ++i) { if (prm->mat[i] < lo) lo = prm->mat[i]; if (prm->mat[i] > hi) hi = prm->mat[i]; }
	*minmat = lo; *maxmat = hi;
	if (bias) *bias = (prm->score_size == 0 || prm->score_size == 2) ? -lo : 0;
}

/* the empty record: score 0, no begin positions, no CIGAR (what the reference gives an empty sequence, src/ssw.c:900-903) */
static void topk_pad(ssw_gpu_result* o) { memset(o, 0, sizeof *o); o->ref_begin1 = -1; o->read_begin1 = -1; o->cigar_off = -1; }

/* Host CIGAR staging pool of a call: every batch of CIGARs that comes off the device is appended here; records name their CIGAR by its
   word offset in the pool. */
typedef struct { uint32_t* words; int64_t n, cap; } cigar_stage;
static int stage_reserve(ssw_gpu_ctx* c, cigar_stage* st, int64_t extra)
{
	if (st->n + extra <= st->cap) return 0;
	const int64_t ncap = (st->n + extra) * 2 + 1024;
	uint32_t* nw = (uint32_t*)realloc(st->words, sizeof(uint32_t) * (size_t)ncap);
	if (!nw) return fail(c, "out of host memory (%s)", "CIGAR pool");
	st->words = nw; st->cap = ncap;
	return 0;
}
/* What a fallback does after a nested call: the nested call's pool (`pool`, `words`; freed here) joins the stage, its m records rec[] go to
   results[] at the indices idx[0], idx[1], .. (`idx_stride` bytes apart) with cigar_off shifted to the stage */
static int stage_append_batch(ssw_gpu_ctx* c, cigar_stage* st, uint32_t* pool, int64_t words, const ssw_gpu_result* rec, int64_t m,
                              const int64_t* idx, size_t idx_stride, ssw_gpu_result* results)
{
	if (words > 0) {
		if (stage_reserve(c, st, words)) { free(pool); return -1; }
		memcpy(st->words + st->n, pool, sizeof(uint32_t) * (size_t)words);
	}
	free(pool);
	for (int64_t k = 0; k < m; ++k) {
		ssw_gpu_result r = rec[k];
		if (r.cigarLen > 0 && r.cigar_off >= 0) r.cigar_off += st->n;
		results[*(const int64_t*)((const char*)idx + idx_stride * (size_t)k)] = r;
	}
	st->n += words;
	return 0;
}
/* CIGARs of cnt downloaded records (hres; d_res on the device, their slots in d_cig) on their way into the stage.  goffs[k]: where record
   k's CIGAR starts, in words from st->n -- the caller advances st->n by *gwords once its records name them.  The used slots are packed into
   one device pool (k_gather) and come down in one copy, enqueued on the main stream and not waited for.  direct: every CIGAR straight from
   its slot instead (a handful of alignments: no offset upload, no gather launch). */
static int cigars_to_stage(ssw_gpu_ctx* c, const ssw_dres* hres, int32_t cnt, const ssw_dres* d_res, const uint32_t* d_cig, cigar_stage* st,
                           int64_t* goffs, int direct, int64_t* gwords)
{
	int64_t at = 0;
	for (int32_t k = 0; k < cnt; ++k) { goffs[k] = at; if (hres[k].cigarLen > 0 && hres[k].status == 0) at += hres[k].cigarLen; }
	*gwords = at;
	if (at == 0) return 0;
	int64_t* d_goff = (int64_t*)ensure(c, &c->goff, sizeof(int64_t) * (size_t)cnt);
	uint32_t* d_gpool = (uint32_t*)ensure(c, &c->gpool, sizeof(uint32_t) * (size_t)at);
	if (!d_goff || !d_gpool || stage_reserve(c, st, at)) return -1;
	if (direct) {
		for (int32_t k = 0; k < cnt; ++k)
			if (hres[k].cigarLen > 0 && hres[k].status == 0 &&
			    ssw_shim_d2h(st->words + st->n + goffs[k], d_cig + hres[k].cigar_off, sizeof(uint32_t) * (size_t)hres[k].cigarLen, c->stream))
				return fail(c, "CIGAR download failed: %s", ssw_shim_last_error());
		return 0;
	}
	ssw_gather_args ga; ga.src = d_cig; ga.res = d_res; ga.dst_off = d_goff; ga.dst = d_gpool; ga.nq = cnt;
	if (ssw_shim_h2d(d_goff, goffs, sizeof(int64_t) * (size_t)cnt, c->stream) || ssw_shim_launch_gather(&ga, c->stream) ||
	    ssw_shim_d2h(st->words + st->n, d_gpool, sizeof(uint32_t) * (size_t)at, c->stream))
		return fail(c, "CIGAR download failed: %s", ssw_shim_last_error());
	return 0;
}

/* sums the timing records of the nested calls of one call; the fill kernel named is the one of the nested call with the most cells */
typedef struct { ssw_gpu_timing t; int64_t best_cells; } call_acc;
static void timing_add(call_acc* acc, const ssw_gpu_timing* t)
{
	ssw_gpu_timing* a = &acc->t;
	a->fill_ms += t->fill_ms; a->fill_launches += t->fill_launches; a->fill_cells += t->fill_cells; a->cells += t->cells;
	a->reduce_ms += t->reduce_ms; a->locate_ms += t->locate_ms; a->trace_ms += t->trace_ms; a->n_word += t->n_word; a->n_byte += t->n_byte;
	a->db_repeats += t->db_repeats; a->fill_pipelined += t->fill_pipelined; a->win_copied += t->win_copied;
	a->db_long_pairs += t->db_long_pairs;
	if (t->fill_cells > acc->best_cells) {
		acc->best_cells = t->fill_cells;
		memcpy(a->fill_kernel, t->fill_kernel, sizeof a->fill_kernel);
		a->fill_ops_per_row = t->fill_ops_per_row; a->fill_rows_per_lane = t->fill_rows_per_lane; a->fill_strips = t->fill_strips;
	}
}

/* queries that share a chain geometry: short queries (<= 384 residues) by R = ceil(len/16) rows per lane, one strip;
   longer ones by their padded length P16, cut into `strips` row strips of lanes*R rows (k_chainx; lanes = 64: the
   wavefront is one chain, 16: four chains per wavefront) */
typedef struct { int32_t R, strips, P16, lanes, use_x; int32_t first_pair, npairs; int32_t first_q, nq; int32_t tailR; /* k_chainq: rows per lane of the last strip (0: R) */
                 int32_t half; /* rows per position R8 = 2R - 1 when every read of the bucket pads to P16 - 8 under 16-bit rules (k_fill8), else 0 */ } bucket;

/* Geometry of the strip kernel and its window passes for an alphabet of n letters.  The forward pass of a batch and the reverse pass over
   flagged survivors (of a database search or of a pair list) must bucket a query length the same way: both take it from here. */
typedef struct {
	int32_t xlanes;      /* lanes of a chain of long queries: 64, the wavefront is one chain (16: four chains per wavefront) */
	int32_t xrmax;       /* most rows per lane of a strip */
	int32_t xrcap;       /* ... of a strip of the window passes */
	int32_t rows;        /* rows of one full strip */
	int no_tail;         /* SSW_GPU_NO_TAIL: equal strips */
} win_geom;
static void win_geom_fill(win_geom* g, const ssw_knobs* kn, int32_t n)
{
	/* long queries: the wavefront is one chain of 64 lanes; rows per lane bounded so that one profile stays near 24 KiB
	   of LDS (several waves per CU).  SSW_GPU_XLANES=16 / SSW_GPU_XR=<rows per lane> override (experiments). */
	g->xlanes = 64; g->xrmax = 4 * (24 / (n + 1) < 1 ? 1 : 24 / (n + 1) > 3 ? 3 : 24 / (n + 1));
	/* measured on 10-kb DNA reads: fill 1462 / 1514 / 1550 / 1604 / 1568 ms at 12 / 11 / 10 / 9 / 8 rows per lane (9..12 share an LDS
	   footprint -- three 16-byte profile chunks per lane and residue --, and the more rows a step has, the less its fixed part
	   weighs; before the record branch was deferred by a step 10 was ahead of 12, profiles/round2_sweep_d_config4_xr*.json vs
	   round2_sweep_o_config4_xr*.json).  The window passes carry two target rings and more registers; round 2 found them fastest at 8 rows per lane.  Measured again in
	   round 6 -- since round 4 the reverse pass walks a diagonal band, where every strip pays 2 x band columns beside its own rows, so fewer, taller strips win: config 4's
	   window passes 138.0 / 112.7 / 101.2 / 86.5 / 85.4 ms at 4 / 6 / 8 / 10 / 12 rows per lane (profiles/round6_experiments.json): 12 */
	g->xrcap = 12;
	if (kn->xlanes16) g->xlanes = 16;
	if (kn->xr) { g->xrmax = kn->xr; g->xrcap = g->xrmax; }
	if (kn->xr_window) g->xrcap = kn->xr_window;
	/* the target rings hold profile offsets as 16-bit values: residue n (the null column) x ceil(R/4) KiB must stay below 64 KiB */
	while (g->xlanes == 64 && g->xrmax > 4 && (int64_t)n * ((g->xrmax + 3) / 4) * 1024 > 65535) g->xrmax -= 4;
	g->rows = g->xlanes * (g->xlanes == 64 ? g->xrmax : SSW_RMAX);
	g->no_tail = kn->no_tail;
}
/* Bucket key of a query of `len` residues, its padded length in *P16q.  Short queries (<= 384): rows per lane R = ceil(len / 16), all queries
   of a bucket have the same padded length.  Long queries of ONE strip (up to 64 x 12 rows): SSW_RMAX + 1 + the rows per lane -- queries of
   DIFFERENT padded lengths share a bucket and its launch (every job of the strip kernel takes its rows from its own queries; rows below a
   query's padded length are dead for its half), sorted by length so that the two queries of a pair mostly have the same one; longer ones:
   SSW_RMAX + 64 + the padded length / 16.  One launch per padded length (round 3) made a batch of mixed long reads a series of small,
   latency-bound launches. */
static int32_t win_bucket_key(const win_geom* g, int32_t len, int32_t* P16q)
{
	const int32_t P = (len + 15) / 16 * 16;
	*P16q = P;
	if (len <= 16 * SSW_RMAX) return P / 16;
	const int32_t st = (P + g->rows - 1) / g->rows, Rq = (P + g->xlanes * st - 1) / (g->xlanes * st);
	/* (only single-strip queries share a bucket across padded lengths: with several strips the 16-bit-rule column maximum -- rows below
	   P8 -- is masked in the job's LAST strip only, which both queries of a pair must then end in) */
	return st == 1 ? SSW_RMAX + 1 + Rq : SSW_RMAX + 64 + P / 16;
}
/* the strip shape of the bucket `key` whose longest query has the padded length P16 */
static void win_bucket_shape(bucket* b, const win_geom* g, int32_t key, int32_t P16)
{
	b->tailR = 0; b->half = 0;
	if (key <= SSW_RMAX) { b->R = key; b->strips = 1; b->P16 = 16 * key; b->lanes = 16; b->use_x = 0; return; }
	b->P16 = P16; b->lanes = g->xlanes; b->use_x = 1;
	b->strips = (P16 + g->rows - 1) / g->rows;
	b->R = (P16 + b->lanes * b->strips - 1) / (b->lanes * b->strips);        /* balanced strips */
	/* ... unless full strips and a SHORT last one (1, 2 or 4 rows per lane) compute fewer rows: 10 000 rows are 13 strips of 768 and one
	   of 64 (10 048 rows) instead of 14 of 768 (10 752).  The last strip pays a step's fixed part (boundary records, hand-offs) again,
	   which is what a strip of 12 rows per lane pays too. */
	if (b->lanes == 64 && b->strips > 1 && g->xrmax > 4 && !g->no_tail) {
		const int32_t rem = P16 - (b->strips - 1) * 64 * g->xrmax, need = (rem + 63) / 64, tr = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : 0;
		if (rem > 0 && tr > 0 && g->xrmax * (b->strips - 1) + tr < b->R * b->strips) { b->R = g->xrmax; b->tailR = tr; }
	}
}

/* tile geometry and scratch of one bucket against the current target (planned before anything is launched: buckets whose launches all
   fit the budget together run side by side on the side streams, each in its own slice of the scratch buffers) */
typedef struct {
	int active, dbl, seg;
	int pipe;                               /* 0, or the number of parts (2 unless a hook says otherwise): the launches of the bucket go round the main stream and the extra one(s), each with its own part of the scratch (below) */
	int32_t tile, halo, ntiles;
	int64_t maxcols, chunk;
	size_t cm_bytes, sg_bytes, bnd_bytes, cand_bytes, q_ints, cs_ints;      /* scratch of one launch */
	size_t cm_off, sg_off, bnd_off, cand_off, q_off, cs_off;                /* its slice when the buckets run side by side, else 0 */
} bplan;
typedef struct { int32_t key, sub, q; } keyed;
typedef struct { int32_t key, need, q; } tpend;     /* traceback negotiation: key = band (wave kernel) or scratch need */
static int tpend_cmp(const void* a, const void* b)
{
	const tpend* x = (const tpend*)a; const tpend* y = (const tpend*)b;
	if (x->key != y->key) return x->key < y->key ? -1 : 1;
	return x->q < y->q ? -1 : x->q > y->q;
}
static int keyed_cmp(const void* a, const void* b)
{
	const keyed* x = (const keyed*)a; const keyed* y = (const keyed*)b;
	if (x->key != y->key) return x->key < y->key ? -1 : 1;
	if (x->sub != y->sub) return x->sub < y->sub ? -1 : 1;
	return x->q < y->q ? -1 : (x->q > y->q);
}

/* VALU instructions of k_fill8<R>'s recurrence per (row, column) of a query pair, counted as chain_row8 / cm_finish8 (ssw_kernels.hip) emit
   them: four per row and one diagonal add per two rows (a 64-bit add on a register pair; the last row of an odd R has its own), F's 4 x gapE
   after every class-3 row but the last, and the column maximum per class -- a maximum of three per two values, a single one for an odd
   value of classes 1 to 3, the three class offsets and the last fold.  R = 19: 103 / 19 = 5.42.  R = 9 is
   the one instance without the blocked row frame (RowFrame8<9>::P in ssw_kernels.hip): the column frame's 6.5.
   dg (gaps from the diagonal): three per row, and per two rows one more 64-bit add, the subtract of gapO - gapE (the last row of an odd R its own).
   R = 19: 94 / 19 = 4.947.  dg == 1, the plain adds in pairs (RowFrame8 in ssw_kernels.hip): one less each for the class offsets of classes 1 and 2
   in one 64-bit subtract (R >= 7), class 3's offset beside F's last subtract (R >= 11) and the last row's diagonal add beside another of F's
   subtracts (R >= 13) -- R = 19: 91 / 19 = 4.789; the floor that shares F's first subtract is no part of the recurrence.  dg == 2 (test hooks): the
   form without the pairs.  The exact counts are in include/ssw_gpu.h.  REPORTED is max(count, 5.0): the row-frame instances are held to
   5.0 <= fill_ops_per_row < 6.5 by their tests */
static double fill8_ops_per_row(int R, int dg)
{
	if (R == 9) return 6.5;
	int cm = 0, last = 1;      /* last: values of the closing fold, class 0 first */
	for (int k = 0; k < 4 && k < R; ++k) {
		const int n = (R - 1 - k) / 4 + 1 + (k == 0);
		cm += (n - 1) / 2;
		if (k == 0) last += (n & 1) == 0;
		else { cm += 1 + ((n & 1) == 0); ++last; }
	}
	const int paired = dg == 1 ? (R >= 7) + (R >= 11) + (R >= 13) : 0;
	const double ops = (double)((dg ? 3 : 4) * R + (dg ? 2 : 1) * ((R + 1) / 2) + (R - 1) / 4 + cm + last / 2 - paired) / R;
	return dg && ops < 5.0 ? 5.0 : ops;
}

/* remembers which fill kernel evaluated most cells of the call (ssw_gpu_timing.fill_kernel) */
static void note_fill_kernel(ssw_gpu_ctx* c, int64_t cells, int64_t* best_cells, const char* name, double ops, int32_t R, int32_t strips)
{
	if (cells <= *best_cells) return;
	*best_cells = cells;
	snprintf(c->tm.fill_kernel, sizeof c->tm.fill_kernel, "%s", name);
	c->tm.fill_ops_per_row = ops; c->tm.fill_rows_per_lane = R; c->tm.fill_strips = strips;
}

/* the error word of this call's work-queue launches: a strip that waited for the one above it for 30 seconds gave up (never seen; it
   would mean a broken queue) and raised it, or -- pair mode -- k_reduce_pairs found a job whose tracked best cell is not the first column
   of its maximum (never seen either: one tile, no halo) -- checked once, before results are handed out.  One word per call, apart from the queue
   buffers: those are reused (and zeroed) from launch to launch without a host round trip. */
static int chainq_check(ssw_gpu_ctx* c)
{
	if (!c->queue_used || !c->qerr.p) return 0;
	int32_t e = 0;
	c->queue_used = 0;
	if (ssw_shim_d2h(&e, c->qerr.p, sizeof e, c->stream) || ssw_shim_stream_sync(c->stream)) return fail(c, "download failed: %s", ssw_shim_last_error());
	if (ssw_shim_memset(c->qerr.p, 0, sizeof e, c->stream)) return fail(c, "memset failed: %s", ssw_shim_last_error());
	return e ? fail(c, "internal error in the strip kernel's work queue: a strip timed out waiting for the strip above it, or a job's best cell "
	                   "disagrees with its column maxima%s", "") : 0;
}

/* work-queue launches of the 64-lane strip kernel (k_chainq): zeroed ticket counter + completion flags (q: items + 2 ints), one best-cell
   record per (job, strip) item (cs: 8 ints per item); both on `stream` */
static size_t chainq_queue_ints(int64_t items) { return (size_t)(items + 2 + 3) / 4 * 4; }
static size_t chainq_cands_ints(int64_t items) { return (size_t)8 * (size_t)(items > 0 ? items : 1); }
static int chainq_setup(ssw_gpu_ctx* c, ssw_chainx_args* xa, int32_t strips, int64_t jobs, int64_t slots_hint, int32_t* q, int32_t* cs, void* stream)
{
	const int64_t items = jobs * strips;
	if (!c->qerr.p) {
		if (!ensure(c, &c->qerr, 16) || ssw_shim_memset(c->qerr.p, 0, 16, c->stream) || ssw_shim_stream_sync(c->stream)) return fail(c, "memset failed: %s", ssw_shim_last_error());
	}
	if (ssw_shim_memset(q, 0, sizeof(int32_t) * (size_t)(items + 2), stream)) return fail(c, "memset failed: %s", ssw_shim_last_error());
	xa->strips = strips; xa->queue = q; xa->cand_strip = cs; xa->err = (int32_t*)c->qerr.p;
	c->queue_used = 1;
	/* strip-level tickets pay off when there are more jobs than wavefront slots (the last round of whole jobs would leave slots
	   idle); with fewer jobs every wavefront keeps its job: SSW_GPU_QUEUE=strips / jobs forces one or the other */
	{
		const int64_t slots = slots_hint > 0 ? slots_hint : (c->dev_wave_slots > 0 ? c->dev_wave_slots : 2048);
		xa->whole_jobs = c->kn.queue_mode == 1 ? 1 : c->kn.queue_mode == 2 ? 0 : jobs <= slots;
	}
	return 0;
}
static int chainq_prepare(ssw_gpu_ctx* c, ssw_chainx_args* xa, int32_t strips, int64_t jobs, int64_t slots_hint)
{
	const int64_t items = jobs * strips;
	int32_t* q = (int32_t*)ensure(c, &c->queue, sizeof(int32_t) * chainq_queue_ints(items));
	int32_t* cs = (int32_t*)ensure(c, &c->cands, sizeof(int32_t) * chainq_cands_ints(items));
	if (!q || !cs) return -1;
	return chainq_setup(c, xa, strips, jobs, slots_hint, q, cs, c->stream);
}

/* wavefronts of the persistent launch: what the device holds at once (a wavefront that finds the queue empty just ends) */
static int chainq_grid(const ssw_gpu_ctx* c, int R, int capture, int n)
{
	if (c->kn.queue_waves > 0) return c->kn.queue_waves;
	const int res = ssw_shim_chainq_resident(R, capture, n);
	if (c->kn.debug) fprintf(stderr, "[ssw_gpu] k_chainq<%d,%s>: %d wavefronts resident on the device\n", R, capture ? "window" : "fill", res);
	return res > 0 ? res : 4096;
}

static int launch_window_pass(ssw_gpu_ctx* c, int32_t R, int32_t lanes, int32_t strips, ssw_chainx_args* xa, int32_t n)
{
	if (lanes != 64) return ssw_shim_launch_chainx(R, 1, xa, c->stream);
	const int qgrid = chainq_grid(c, R, 1, n);
	if (chainq_prepare(c, xa, strips, ((int64_t)xa->njobs + 1) / 2, qgrid)) return -1;
	if (c->kn.debug) fprintf(stderr, "[ssw_gpu] chainq window pass (reverse %d): R %d, %d queries x %d strips, %d wavefronts, %s tickets, form %d\n",
	                                     xa->reverse, R, xa->njobs, strips, qgrid, xa->whole_jobs ? "job" : "strip", xa->form);
	const int rc = ssw_shim_launch_chainq(R, 1, xa, qgrid, c->stream);
	if (c->kn.debug) { const int src = ssw_shim_stream_sync(c->stream); fprintf(stderr, "[ssw_gpu] chainq window pass done (sync rc %d: %s)\n", src, src ? ssw_shim_last_error() : "ok"); }
	return rc;
}

/*
 * Database-search path: many short targets, flag == 0.  One fused launch (k_filldb) per (bucket, target chunk) instead
 * of three launches per target; targets are sorted by length so that the 16 chains of a workgroup finish together.
 */
typedef struct { int32_t len, t; } tkey;
static int tkey_cmp(const void* a, const void* b)
{
	const tkey* x = (const tkey*)a; const tkey* y = (const tkey*)b;
	if (x->len != y->len) return x->len < y->len ? -1 : 1;
	return x->t < y->t ? -1 : (x->t > y->t);
}

/* select mode of the streamed search (ssw_gpu_search_topk): k_topk merges every chunk into per-query lists on the second stream */
typedef struct {
	ssw_topk_args a;                    /* lists, k, key buffer, min_score (hits / nt / tfirst are set per chunk) */
	void** ev; int nev;                 /* an event pair around the selection of every chunk (2 x chunks, created by the caller) */
} topk_sel;

/* streamed database search (ssw_gpu_search_db): compact records of one target chunk go to one of two device buffers, are
   downloaded on the second stream into one of two page-locked host buffers while the next chunk is computed, and are handed
   to the caller's function -- or, in select mode (fn == NULL, sel set), stay on the device for k_topk */
typedef struct {
	int32_t chunk;                      /* targets per chunk */
	ssw_gpu_hits_fn fn; void* user;
	topk_sel* sel;
	struct ssw_hit_rec* d_hits[2];
	ssw_gpu_hit* h_hits[2];
	int fn_rc;                          /* non-zero: the caller's function asked to stop */
	size_t cnt_off;                     /* byte offset in h_hits[]: snapshot of the device counters taken after the chunk */
} db_stream;

#define DB_COUNTERS 4                   /* [0] 16-bit-rule alignments, [1] 8-bit-rule, [2] workgroups of k_filldb that repeated in the int16 form */


/* Flagged database search (round 4): begin positions / CIGARs against MANY targets in one batch call -- the reference's loop calls
   ssw_align with flag 2 and a score filter for every (read, target) pair (src/main.c:493-506; gating src/ssw.c:916, 938).  Scores and end
   positions of all pairs of a chunk of targets come from k_filldb exactly as in the score-only search; k_select compacts the pairs that
   pass ssw.c:916 into a survivor list (ordered by geometry bucket, query, target); ONE batched reverse pass per bucket and one
   traceback negotiation then run over the survivors as (query, target) jobs (ssw_vmap) -- no per-target loop, no per-target sync. */
typedef struct {
	const int32_t* order; int32_t nqa;     /* non-empty queries in bucket order (host), and ... */
	const int32_t* d_order;                /* ... on the device */
	int32_t maxlen, maxmat, minmat, maxt;
	win_geom g;
	int fill_form;
	cigar_stage* stage;                    /* the call's host CIGAR pool */
	double locate_ms, trace_ms;
	int64_t survivors;
	/* survivors of the current chunk, on the host after dbx_chunk */
	ssw_dres* hs; int32_t* hvq; int32_t* hvt; int64_t* hpo; int32_t ns; size_t hcap;
} dbx_state;
static int dbx_chunk(ssw_gpu_ctx* c, dbx_state* dx, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const ssw_gpu_params* prm, const bucket* bk, int nb,
                     const int8_t* d_mat, struct ssw_out_rec* d_out, int32_t tbase, int32_t nt);

/* scratch of ONE job of the strip kernel's pair mode against a target of tl columns: two rows of column maxima, the boundary records of the
   strip hand-off, queue flag + best-cell record per strip, the job's best cells and its two records */
static int64_t plong_cm_stride(int64_t tl) { return (tl + 15) / 16 * 16 + 16; }
static int64_t plong_bnd_cols(int64_t tl) { return (tl + 31) / 16 * 16; }
static int64_t plong_job_bytes(int64_t tl, int32_t strips)
{
	return 8 * plong_cm_stride(tl) + 16 * plong_bnd_cols(tl) + 36 * (int64_t)strips + 32 + 2 * (int64_t)sizeof(ssw_gpu_result);
}

/* The long class of the database path: queries above k_filldb's classes (641 residues and more; 385 and more where the alphabet keeps the
   classes of 25..40 rows per lane out) on the strip kernel's pair mode.  A job is (q, ta, q, tb): BOTH halves of a register hold the same
   query, against two neighbours of the chunk's length-sorted targets -- the partner of identical padded length that jobs of several strips
   need is the query itself.  k_dbjobs writes the jobs of a launch on the device, k_reduce_pairs (database mode) stores the records in the
   chunk's matrix beside k_filldb's.  qdone[q] == 2 marks the class's queries. */
#define PJ_LONG_MAX 65535      /* longest query of the pair mode, here and on the pair path */
typedef struct {
	int nlb;
	bucket* b;                            /* [nlb] strip shapes (win_bucket_shape); first_q / nq: the bucket's slice of the call's bucket-ordered query list */
	int64_t* cells;                       /* [nlb] cells evaluated, summed over the chunks */
	int* form;                            /* [nlb] 3: column frame, 0: plain int16 */
	const int32_t* d_order;               /* that list on the device */
	int32_t maxmat, minmat;
} dbl_class;

/* one chunk's launches of the long class, on the main stream: nz non-empty targets d_tl (host copy tl) in length order */
static int dbl_chunk(ssw_gpu_ctx* c, dbl_class* dl, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const ssw_gpu_params* prm, const int8_t* d_mat, int32_t bias,
                     int32_t maxtlen, const int32_t* d_tl, const int32_t* tl, int32_t nz, int32_t tfirst, int32_t res_nt,
                     ssw_dres* d_res, struct ssw_out_rec* d_out, struct ssw_hit_rec* d_hits, int32_t* d_cnt, int mark_word)
{
	const int32_t n = prm->n;
	const uint32_t gapO2 = (uint32_t)prm->gapO * 0x10001u, gapE2 = (uint32_t)prm->gapE * 0x10001u;
	const int64_t hp = ((int64_t)nz + 1) / 2;
	const int64_t stride = plong_cm_stride(maxtlen), bcols = plong_bnd_cols(maxtlen);
	int64_t colsum = 0;      /* columns a row of jobs walks: the longer target of every job (sorted: the second one) */
	for (int64_t p = 0; p < hp; ++p) { const int32_t t = tl[2 * p + 1 < nz ? 2 * p + 1 : 2 * p]; colsum += T->h_off[t + 1] - T->h_off[t]; }
	for (int b = 0; b < dl->nlb; ++b) {
		const bucket* B = &dl->b[b];
		const int64_t total = (int64_t)B->nq * hp;
		int64_t jpl = (int64_t)(c->cm_budget / 2) / plong_job_bytes(maxtlen, B->strips);      /* (>= 1: the class's gate) */
		if (jpl < 1) jpl = 1;
		if (jpl > total) jpl = total;
		if (jpl * B->strips > 0x7ffffff0 / 2) jpl = 0x7ffffff0 / 2 / B->strips;
		uint32_t* d_cm16 = (uint32_t*)ensure(c, &c->cm16, (size_t)(4 * stride * jpl));
		uint32_t* d_cm8 = (uint32_t*)ensure(c, &c->cm8, (size_t)(4 * stride * jpl));
		uint32_t* d_bnd = (uint32_t*)ensure(c, &c->bnd, (size_t)(16 * bcols * jpl));
		int32_t* d_cand = (int32_t*)ensure(c, &c->cand, (size_t)(32 * jpl));
		ssw_pjob* d_jobs = (ssw_pjob*)ensure(c, &c->dbjobs, sizeof(ssw_pjob) * (size_t)jpl);
		if (!d_cm16 || !d_cm8 || !d_bnd || !d_cand || !d_jobs) return -1;
		int32_t fr_base = 0, fr_kmask = 0;
		const int xform = !c->kn.fill_plain && !c->kn.db_plain &&
		                  ssw_frame_params(&c->kn, (int64_t)B->P16 * (dl->maxmat > 0 ? dl->maxmat : 0), prm->gapO, prm->gapE, dl->minmat, 64, &fr_base, &fr_kmask) ? 3 : 0;
		dl->form[b] = xform;
		const int qgrid = chainq_grid(c, B->R, 1, n);      /* (the window pass's occupancy, as the pair path's long class: the same LDS footprint) */
		for (int64_t a0 = 0; a0 < total; a0 += jpl) {
			const int64_t nl = total - a0 < jpl ? total - a0 : jpl;
			ssw_dbjobs_args ja; memset(&ja, 0, sizeof ja);
			ja.qlist = dl->d_order + B->first_q; ja.tlist = d_tl; ja.ntl = nz; ja.first = a0; ja.count = nl; ja.jobs = d_jobs;
			if (ssw_shim_launch_dbjobs(&ja, c->stream)) return fail(c, "job list launch failed: %s", ssw_shim_last_error());
			ssw_chainx_args xa; memset(&xa, 0, sizeof xa);
			xa.qcodes = Q->d_codes; xa.qoff = Q->d_off; xa.mat = d_mat; xa.n = n; xa.gapO2 = gapO2; xa.gapE2 = gapE2; xa.gapE = prm->gapE; xa.maxmat = dl->maxmat;
			xa.njobs = (int32_t)nl; xa.pjobs = d_jobs; xa.vm.tcodes = T->d_codes; xa.vm.toff = T->d_off;
			xa.ntiles = 1; xa.cm16 = d_cm16; xa.cm8 = d_cm8; xa.cm_stride = stride; xa.bnd = d_bnd; xa.bnd_stride = bcols; xa.cand = d_cand; xa.lanes = 64;
			if (chainq_prepare(c, &xa, B->strips, nl, qgrid)) return -1;
			xa.form = xform; xa.fr_base = fr_base; xa.fr_kmask = fr_kmask; xa.tail_R = B->tailR;
			if (c->kn.debug) fprintf(stderr, "[ssw_gpu] database search, long class: R %d (last strip %d), %lld jobs x %d strips, %d wavefronts, %s tickets, form %d\n",
			                                     B->R, B->tailR ? B->tailR : B->R, (long long)nl, B->strips, qgrid, xa.whole_jobs ? "job" : "strip", xa.form);
			if (ssw_shim_launch_chainq(B->R, 2, &xa, qgrid, c->stream)) return fail(c, "fill launch failed: %s", ssw_shim_last_error());
			ssw_reduce_pairs_args ra; memset(&ra, 0, sizeof ra);
			ra.jobs = d_jobs; ra.njobs = xa.njobs; ra.qoff = Q->d_off; ra.toff = T->d_off; ra.cm16 = d_cm16; ra.cm8 = d_cm8; ra.cm_stride = stride;
			ra.cand = d_cand; ra.maskLen = prm->maskLen; ra.bias = bias; ra.score_size = prm->score_size; ra.counters = d_cnt; ra.mark_word = mark_word; ra.err = xa.err;
			ra.res_nt = res_nt; ra.tfirst = tfirst; ra.db_hits = d_hits; ra.db_out = d_hits ? 0 : d_out; ra.db_res = d_hits || d_out ? 0 : d_res;
			if (ssw_shim_launch_reduce_pairs(&ra, c->stream)) return fail(c, "reduce launch failed: %s", ssw_shim_last_error());
		}
		const int64_t rows = (int64_t)64 * (B->tailR ? B->R * (B->strips - 1) + B->tailR : B->R * B->strips);
		const int64_t bcells = rows * 2 * colsum * B->nq;
		c->tm.fill_cells += bcells; dl->cells[b] += bcells;
		c->tm.db_long_pairs += (int64_t)B->nq * nz;
	}
	return 0;
}

static int align_db(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, int32_t tfirst, int32_t tcount,
                    const ssw_gpu_params* prm, ssw_gpu_result* results, const bucket* bk, int nb, const ssw_pair* d_pairs,
                    const int8_t* d_mat, int32_t bias, int32_t maxtlen, const uint8_t* qdone, db_stream* ds, dbx_state* dx, dbl_class* dl)
{
	const int32_t nq = Q->count, n = prm->n;
	const uint32_t gapO2 = (uint32_t)prm->gapO * 0x10001u, gapE2 = (uint32_t)prm->gapE * 0x10001u;
	const int64_t stride = ((int64_t)maxtlen + 15) / 16 * 16 + 16;
	int rc = -1;
	tkey* tk = (tkey*)malloc(sizeof(tkey) * (size_t)tcount);
	int32_t* tl_all = (int32_t*)malloc(sizeof(int32_t) * (size_t)tcount);
	ssw_dres* hres = 0;
	if (!tk || !tl_all) { free(tk); free(tl_all); return fail(c, "out of host memory%s", ""); }
	/* queries of 385..640 residues: still one strip of the fused kernel, classes R = ceil(len / 16) = 25..40 like the short ones
	   (the profile offsets of the target ring are 16-bit: alphabets whose null column would lie beyond 64 KiB keep these queries on
	   the per-target path) */
	bucket mid[16]; int nmid = 0;
	ssw_pair* midpairs = 0; const ssw_pair* d_midpairs = 0;
	{
		int32_t nm = 0;
		for (int32_t q = 0; q < nq; ++q) if (qdone[q] == 1) { const int64_t L = Q->h_off[q + 1] - Q->h_off[q]; if (L > 16 * SSW_RMAX && L <= 640) ++nm; }
		if (nm > 0) {
			keyed* mk = (keyed*)malloc(sizeof(keyed) * (size_t)nm);
			midpairs = (ssw_pair*)malloc(sizeof(ssw_pair) * (size_t)nm);
			if (!mk || !midpairs) { free(mk); free(midpairs); free(tk); free(tl_all); return fail(c, "out of host memory%s", ""); }
			int32_t k = 0, np = 0;
			for (int32_t q = 0; q < nq; ++q) if (qdone[q] == 1) { const int64_t L = Q->h_off[q + 1] - Q->h_off[q]; if (L > 16 * SSW_RMAX && L <= 640) { mk[k].key = (int32_t)L; mk[k].sub = 0; mk[k].q = q; ++k; } }
			qsort(mk, (size_t)nm, sizeof(keyed), keyed_cmp);
			for (int cls = SSW_RMAX + 1; cls <= 40; ++cls) {
				bucket b; b.tailR = 0; b.R = cls; b.strips = 1; b.P16 = 16 * cls; b.lanes = 16; b.use_x = 0; b.first_pair = np; b.first_q = 0; b.nq = 0;
				for (int32_t i = 0; i < nm; ++i) {      /* sorted by length: the queries of a class are contiguous; neighbours share a chain */
					if ((mk[i].key + 15) / 16 != cls) continue;
					midpairs[np].qa = mk[i].q; midpairs[np].qb = -1; ++b.nq;
					if (i + 1 < nm && (mk[i + 1].key + 15) / 16 == cls) { midpairs[np].qb = mk[i + 1].q; ++b.nq; ++i; }
					++np;
				}
				b.npairs = np - b.first_pair;
				if (b.npairs > 0) mid[nmid++] = b;
			}
			free(mk);
			ssw_pair* dmp = (ssw_pair*)ensure(c, &c->pairs2, sizeof(ssw_pair) * (size_t)np);
			if (!dmp || ssw_shim_h2d(dmp, midpairs, sizeof(ssw_pair) * (size_t)np, c->stream)) { free(midpairs); free(tk); free(tl_all); return fail(c, "upload failed: %s", ssw_shim_last_error()); }
			d_midpairs = dmp;
		}
	}
	/* result records of a sub-batch of targets stay in HBM until the sub-batch is done */
	int64_t tsub = (int64_t)(c->cm_budget / 2) / ((int64_t)nq * (int64_t)sizeof(ssw_dres));
	if (dx) tsub = (int64_t)(c->cm_budget / 4) / ((int64_t)nq * (int64_t)sizeof(struct ssw_out_rec));
	if (tsub < 16) tsub = 16;
	if (c->kn.db_tsub) tsub = c->kn.db_tsub;
	if (ds) tsub = ds->chunk;
	if (tsub > tcount) tsub = tcount;
	int32_t* d_tl_all = (int32_t*)ensure(c, &c->tlist, sizeof(int32_t) * (size_t)tcount);     /* every sub-batch has its own slice (uploads stay in flight) */
	int32_t* d_cnt_s = ds ? (int32_t*)ensure(c, &c->need, DB_COUNTERS * sizeof(int32_t)) : 0;
	const int nch = SSW_DB_NCH;
	/* column-frame form of the recurrence wherever a size class's scores leave room for the frame offsets below 31744 (always, for the
	   matrices and lengths this path admits with sane gap penalties); SSW_GPU_DB_FORM=0 (tests) keeps the plain int16 form */
	const int use_fr = !c->kn.db_plain;
	int32_t db_minmat, db_maxmat;
	mat_range(prm, &db_minmat, &db_maxmat, 0);
	int db_form[64]; memset(db_form, 0, sizeof db_form);
	if (!d_tl_all || (ds && (!d_cnt_s || ssw_shim_memset(d_cnt_s, 0, DB_COUNTERS * sizeof(int32_t), c->stream)))) { fail(c, "device allocation failed: %s", ssw_shim_last_error()); goto done; }
	int32_t prev_t0 = -1, prev_nt = 0, chunk_i = 0;
	int64_t db_cells[64]; memset(db_cells, 0, sizeof db_cells);      /* per bucket (nb <= 24 short buckets + up to 16 classes of 385..640 residues) */
	for (int32_t t0 = 0; t0 < tcount; t0 += (int32_t)tsub, ++chunk_i) {
		const int32_t nt = tcount - t0 < tsub ? tcount - t0 : (int32_t)tsub;
		int32_t* const tl = tl_all + t0;
		for (int32_t k = 0; k < nt; ++k) { tk[k].t = tfirst + t0 + k; tk[k].len = (int32_t)(T->h_off[tfirst + t0 + k + 1] - T->h_off[tfirst + t0 + k]); }
		qsort(tk, (size_t)nt, sizeof(tkey), tkey_cmp);
		int32_t nz = 0;
		for (int32_t k = 0; k < nt; ++k) if (tk[k].len > 0) tl[nz++] = tk[k].t;      /* empty targets keep their zeroed records */
		/* one sub-batch covering every target and every query handled here: the kernel writes final-layout records that are
		   downloaded straight into the caller's array (no host-side conversion pass over nq x nt records) */
		int direct = nt == tcount && !ds;
		for (int32_t q = 0; q < nq && direct; ++q) if (!qdone[q]) direct = 0;
		if (dx) direct = 1;      /* final-layout records per chunk; rows of queries that are not handled here stay empty records (the per-target path fills them in later) */
		ssw_dres* d_res = 0; struct ssw_out_rec* d_out = 0; int32_t* d_cnt = 0; struct ssw_hit_rec* d_hits = 0;
		const int buf = chunk_i & 1;
		if (ds) {      /* all-zero bytes ARE the empty compact record (score 0, ends 0): empty queries / targets need no patching */
			d_hits = ds->d_hits[buf]; d_cnt = d_cnt_s;
			/* select mode: the selection that last read this buffer (two chunks back) must be done -- a wait of the stream, not of the host */
			if (ds->sel && chunk_i >= 2 && ssw_shim_stream_wait_event(c->stream, c->ev_red[buf])) { fail(c, "stream wait failed: %s", ssw_shim_last_error()); goto done; }
			if (ssw_shim_memset(d_hits, 0, sizeof(struct ssw_hit_rec) * (size_t)nq * (size_t)nt, c->stream)) { fail(c, "memset failed: %s", ssw_shim_last_error()); goto done; }
		} else
		if (direct) {
			d_out = (struct ssw_out_rec*)ensure(c, &c->res, sizeof(struct ssw_out_rec) * (size_t)nq * (size_t)nt);
			d_cnt = (int32_t*)ensure(c, &c->need, DB_COUNTERS * sizeof(int32_t));
			if (!d_out || !d_cnt) goto done;
			/* all-zero bytes are not a valid empty record (begins are -1): empty targets are patched on the host below */
			if (ssw_shim_memset(d_out, 0, sizeof(struct ssw_out_rec) * (size_t)nq * (size_t)nt, c->stream) ||
			    ssw_shim_memset(d_cnt, 0, DB_COUNTERS * sizeof(int32_t), c->stream)) { fail(c, "memset failed: %s", ssw_shim_last_error()); goto done; }
		} else {
			d_res = (ssw_dres*)ensure(c, &c->res, sizeof(ssw_dres) * (size_t)nq * (size_t)nt);
			if (!d_res || ssw_shim_memset(d_res, 0, sizeof(ssw_dres) * (size_t)nq * (size_t)nt, c->stream)) { fail(c, "memset failed: %s", ssw_shim_last_error()); goto done; }
		}
		int32_t* d_tl = d_tl_all + t0;
		if (ssw_shim_h2d(d_tl, tl, sizeof(int32_t) * (size_t)nz, c->stream)) { fail(c, "upload failed: %s", ssw_shim_last_error()); goto done; }
		/* The size classes of a chunk are independent launches (different query pairs, the same targets): they go round-robin
		   to DB_STREAMS side streams, largest first, so that the tail of one class and the under-filled launches of the rare
		   classes overlap with other classes' work (measured: 23 classes x 4 chunks one after the other cost 25 % more than the
		   same work in 23 launches).  Every stream has its own slice of the column-maximum scratch. */
		void* e0 = next_event(c); void* e1 = next_event(c);
		ssw_shim_event_record(e0, c->stream);
		if (nz > 0) {
			int ord[64], nord = 0, used[DB_STREAMS];
			for (int b = 0; b < nb + nmid && nord < 64; ++b) { const bucket* B = b < nb ? &bk[b] : &mid[b - nb]; if (!B->use_x) ord[nord++] = b; }
			for (int i = 1; i < nord; ++i) {     /* by cells, descending */
				const int v = ord[i]; int j = i;
				const bucket* Bv = v < nb ? &bk[v] : &mid[v - nb];
				while (j > 0) {
					const bucket* Bj = ord[j - 1] < nb ? &bk[ord[j - 1]] : &mid[ord[j - 1] - nb];
					if ((int64_t)Bj->npairs * Bj->P16 >= (int64_t)Bv->npairs * Bv->P16) break;
					ord[j] = ord[j - 1]; --j;
				}
				ord[j] = v;
			}
			const int64_t slice = (int64_t)(c->cm_budget / 2) / (2 * DB_STREAMS) / 16 * 16;      /* bytes of one stream's cm16 (and cm8) slice */
			int64_t need = 0;
			for (int i = 0; i < nord; ++i) {
				const bucket* B = ord[i] < nb ? &bk[ord[i]] : &mid[ord[i] - nb];
				const int64_t w = 4 * stride * (int64_t)nz * B->npairs;
				if (w > need) need = w;
			}
			if (need > slice) need = slice;
			if (need < 4 * stride * nch) need = 4 * stride * nch;     /* ... but never less than one workgroup (one pair x its 16 targets); a class
			                                                             whose pairs do not fit a slice is cut into launches of fewer pairs */
			uint32_t* d_cm16_all = (uint32_t*)ensure(c, &c->cm16, (size_t)(need * DB_STREAMS));
			uint32_t* d_cm8_all = (uint32_t*)ensure(c, &c->cm8, (size_t)(need * DB_STREAMS));
			if (!d_cm16_all || !d_cm8_all) goto done;
			if (ssw_shim_event_record(c->ev_db, c->stream)) { fail(c, "event record failed: %s", ssw_shim_last_error()); goto done; }
			for (int sx = 0; sx < DB_STREAMS; ++sx) used[sx] = 0;
			for (int i = 0; i < nord; ++i) {
				const int b = ord[i], sx = i % DB_STREAMS;
				const bucket* B = b < nb ? &bk[b] : &mid[b - nb];
				const ssw_pair* bpairs = b < nb ? d_pairs : d_midpairs;
				void* st = c->tstream[sx];
				if (!used[sx]) { used[sx] = 1; if (ssw_shim_stream_wait_event(st, c->ev_db)) { fail(c, "stream wait failed: %s", ssw_shim_last_error()); goto done; } }
				/* pairs per launch: all of the class when one workgroup row of them fits the slice, else what fits (the scratch of a launch
				   is 8 bytes x stride x pairs x targets); targets per launch: what the slice then holds, in workgroups of 16 */
				int64_t ppl = B->npairs;
				if (4 * stride * nch * ppl > need) ppl = need / (4 * stride * nch);
				if (ppl < 1) ppl = 1;
				int64_t per = need / (4 * stride * ppl);
				per = per / nch * nch; if (per < nch) per = nch;
				if ((int64_t)4 * stride * per * ppl > need) { fail(c, "database search: %s", "a size class does not fit the column-maximum budget (SSW_GPU_CM_BUDGET_MB)"); goto done; }
				uint32_t* d_cm16 = d_cm16_all + (need / 4) * sx;
				uint32_t* d_cm8 = d_cm8_all + (need / 4) * sx;
				int32_t fr_base = 0, fr_kmask = 0;
				const int fr = use_fr && ssw_frame_params(&c->kn, (int64_t)B->P16 * db_maxmat, prm->gapO, prm->gapE, db_minmat, 16, &fr_base, &fr_kmask);
				if (b < 64) db_form[b] = fr;
				for (int32_t p0 = 0; p0 < B->npairs; p0 += (int32_t)ppl)
				for (int32_t k0 = 0; k0 < nz; k0 += (int32_t)per) {
					ssw_filldb_args fa;
					fa.tcodes = T->d_codes; fa.toff = T->d_off; fa.tlist = d_tl + k0; fa.ntl = nz - k0 < per ? nz - k0 : (int32_t)per;
					fa.tfirst = tfirst + t0; fa.res_nt = nt; fa.qcodes = Q->d_codes; fa.qoff = Q->d_off; fa.pairs = bpairs + B->first_pair + p0;
					fa.npairs = B->npairs - p0 < ppl ? B->npairs - p0 : (int32_t)ppl; fa.mat = d_mat; fa.n = n; fa.gapO2 = gapO2; fa.gapE2 = gapE2; fa.cm16 = d_cm16; fa.cm8 = d_cm8;
					fa.cm_stride = stride; fa.maskLen = prm->maskLen; fa.bias = bias; fa.score_size = prm->score_size; fa.res = d_res; fa.out = d_out; fa.counters = d_cnt;
					fa.hits = d_hits; fa.form = fr; fa.fr_base = fr_base; fa.fr_kmask = fr_kmask; fa.mark_word = dx != 0;
					fa.chain_best = c->kn.db_chain_best;
					if (ssw_shim_launch_filldb(B->R, &fa, st)) { fail(c, "filldb launch failed: %s", ssw_shim_last_error()); goto done; }
					int64_t lc = 0;
					for (int32_t k = 0; k < fa.ntl; ++k)
						lc += (T->h_off[tl[k0 + k] + 1] - T->h_off[tl[k0 + k]]) * (int64_t)B->P16 * 2 * fa.npairs;
					c->tm.fill_cells += lc;
					if (b < 64) db_cells[b] += lc;
				}
			}
			for (int sx = 0; sx < DB_STREAMS; ++sx)
				if (used[sx] && (ssw_shim_event_record(c->tev[sx], c->tstream[sx]) || ssw_shim_stream_wait_event(c->stream, c->tev[sx]))) {
					fail(c, "stream join failed: %s", ssw_shim_last_error()); goto done;
				}
		}
		/* the long class follows on the main stream (its scratch is k_filldb's, free again after the join above): records into the same matrix */
		const int has_long = dl && dl->nlb > 0;
		if (nz > 0 && has_long && dbl_chunk(c, dl, Q, T, prm, d_mat, bias, maxtlen, d_tl, tl, nz, tfirst + t0, nt, d_res, d_out, d_hits, d_cnt, dx != 0)) goto done;
		ssw_shim_event_record(e1, c->stream);
		c->tm.fill_launches++;      /* one launch group: all size classes of this chunk of targets, the long class's launches among them */
		if (ds && ds->sel) {      /* select mode: k_topk on the second stream after this chunk's fill, while the next chunk is computed */
			topk_sel* s = ds->sel;
			s->a.hits = d_hits; s->a.nt = nt; s->a.tfirst = tfirst + t0;
			if (2 * chunk_i + 1 >= s->nev) { fail(c, "top-K selection: %s", "more chunks than planned"); goto done; }
			if (ssw_shim_event_record(c->ev_fill[buf], c->stream) || ssw_shim_stream_wait_event(c->stream2, c->ev_fill[buf]) ||
			    ssw_shim_event_record(s->ev[2 * chunk_i], c->stream2) || ssw_shim_launch_topk(&s->a, c->stream2) ||
			    ssw_shim_event_record(s->ev[2 * chunk_i + 1], c->stream2) || ssw_shim_event_record(c->ev_red[buf], c->stream2)) {
				fail(c, "top-K selection launch failed: %s", ssw_shim_last_error()); goto done;
			}
			prev_t0 = t0; prev_nt = nt;
			continue;
		}
		if (ds) {   /* download of this chunk on the second stream; meanwhile hand the previous chunk to the caller */
			if (ssw_shim_event_record(c->ev_fill[buf], c->stream) || ssw_shim_stream_wait_event(c->stream2, c->ev_fill[buf]) ||
			    ssw_shim_d2h(ds->h_hits[buf], d_hits, sizeof(struct ssw_hit_rec) * (size_t)nq * (size_t)nt, c->stream2) ||
			    ssw_shim_d2h((char*)ds->h_hits[buf] + ds->cnt_off, d_cnt_s, DB_COUNTERS * sizeof(int32_t), c->stream2) ||
			    ssw_shim_event_record(c->ev_red[buf], c->stream2)) { fail(c, "result download failed: %s", ssw_shim_last_error()); goto done; }
			if (prev_t0 >= 0) {
				if (ssw_shim_event_sync(c->ev_red[buf ^ 1])) { fail(c, "result download failed: %s", ssw_shim_last_error()); goto done; }
				ds->fn_rc = ds->fn(ds->user, tfirst + prev_t0, prev_nt, ds->h_hits[buf ^ 1]);
				if (ds->fn_rc) { ssw_shim_stream_sync(c->stream); ssw_shim_stream_sync(c->stream2); rc = 0; goto done; }
			}
			prev_t0 = t0; prev_nt = nt;
			continue;
		}
		if (direct) {
			int32_t cnt[DB_COUNTERS] = { 0, 0, 0, 0 };
			if (dx) {      /* survivors of this chunk: reverse pass, traceback, CIGARs in the host pool.  (The counters first: the phases below regrow c->need.) */
				if (ssw_shim_d2h(cnt, d_cnt, sizeof cnt, c->stream) || ssw_shim_stream_sync(c->stream)) { fail(c, "result download failed: %s", ssw_shim_last_error()); goto done; }
				if (dbx_chunk(c, dx, Q, T, prm, bk, nb, d_mat, d_out, tfirst + t0, nt)) goto done;
			}
			if (nt == tcount) {
				if (ssw_shim_d2h(results, d_out, sizeof(struct ssw_out_rec) * (size_t)nq * (size_t)nt, c->stream)) { fail(c, "result download failed: %s", ssw_shim_last_error()); goto done; }
			} else {      /* a chunk of the targets: every query's slice of the chunk goes to its row */
				for (int32_t q = 0; q < nq; ++q)
					if (ssw_shim_d2h(&results[(int64_t)q * tcount + t0], d_out + (int64_t)q * nt, sizeof(struct ssw_out_rec) * (size_t)nt, c->stream)) {
						fail(c, "result download failed: %s", ssw_shim_last_error()); goto done;
					}
			}
			if ((!dx && ssw_shim_d2h(cnt, d_cnt, sizeof cnt, c->stream)) || ssw_shim_stream_sync(c->stream)) {
				fail(c, "result download failed: %s", ssw_shim_last_error()); goto done;
			}
			c->tm.n_word += cnt[0]; c->tm.n_byte += cnt[1]; c->tm.db_repeats += cnt[2];
			int64_t qsum = 0;
			for (int32_t q = 0; q < nq; ++q) if (qdone[q]) qsum += Q->h_off[q + 1] - Q->h_off[q];      /* (the per-target path counts the cells of the others) */
			for (int32_t k = 0; k < nt; ++k) {
				const int64_t L = T->h_off[tfirst + t0 + k + 1] - T->h_off[tfirst + t0 + k];
				c->tm.cells += qsum * L;
				if (L == 0) for (int32_t q = 0; q < nq; ++q) { ssw_gpu_result* o = &results[(int64_t)q * tcount + t0 + k]; o->ref_begin1 = -1; o->read_begin1 = -1; o->cigar_off = -1; }
			}
			for (int32_t q = 0; q < nq; ++q)      /* empty queries: no kernel wrote their rows */
				if (Q->h_off[q + 1] == Q->h_off[q])
					for (int32_t k = 0; k < nt; ++k) { ssw_gpu_result* o = &results[(int64_t)q * tcount + t0 + k]; o->ref_begin1 = -1; o->read_begin1 = -1; o->cigar_off = -1; }
			if (dx)      /* what the reverse pass and the traceback added to the survivors' records */
				for (int32_t v = 0; v < dx->ns; ++v) {
					const ssw_dres* r = &dx->hs[v];
					ssw_gpu_result* o = &results[(int64_t)dx->hvq[v] * tcount + (dx->hvt[v] - tfirst)];
					o->ref_begin1 = r->ref_begin1; o->read_begin1 = r->read_begin1; o->cigarLen = r->cigarLen; o->flag = (uint16_t)r->flag;
					o->edit_distance = r->nm; o->cigar_off = r->cigarLen > 0 ? dx->hpo[v] : -1;
				}
			continue;
		}
		if (!hres) {     /* only the sub-batched path converts records on the host (the direct path downloads final-layout records) */
			hres = (ssw_dres*)malloc(sizeof(ssw_dres) * (size_t)nq * (size_t)tsub);
			if (!hres) { fail(c, "out of host memory (%s)", "database-search record staging"); goto done; }
		}
		if (ssw_shim_d2h(hres, d_res, sizeof(ssw_dres) * (size_t)nq * (size_t)nt, c->stream) || ssw_shim_stream_sync(c->stream)) {
			fail(c, "result download failed: %s", ssw_shim_last_error()); goto done;
		}
		for (int32_t q = 0; q < nq; ++q)
			for (int32_t k = 0; k < nt && qdone[q]; ++k) {
				const ssw_dres* r = &hres[(int64_t)q * nt + k];
				ssw_gpu_result* o = &results[(int64_t)q * tcount + t0 + k];
				o->score1 = (uint16_t)r->score1; o->score2 = (uint16_t)r->score2; o->ref_begin1 = -1; o->ref_end1 = r->ref_end1;
				o->read_begin1 = -1; o->read_end1 = r->read_end1; o->ref_end2 = r->ref_end2; o->cigarLen = 0; o->edit_distance = 0; o->cigar_off = -1;
				o->flag = 0; o->status = (uint16_t)r->status;
				if (r->status == 0 && r->score1 > 0) { if (r->word) c->tm.n_word++; else c->tm.n_byte++; }
				c->tm.cells += (Q->h_off[q + 1] - Q->h_off[q]) * (T->h_off[tfirst + t0 + k + 1] - T->h_off[tfirst + t0 + k]);
			}
	}
	{
		int64_t bestc = 0;
		for (int b = 0; b < nb + nmid && b < 64; ++b) {
			const bucket* B = b < nb ? &bk[b] : &mid[b - nb];
			char nm[48];
			snprintf(nm, sizeof nm, "k_filldb<%d,%s>", B->R, db_form[b] ? "frame" : "int16+max3");
			note_fill_kernel(c, db_cells[b], &bestc, nm, db_form[b] ? 6.5 : 8.5, B->R, 1);
		}
		for (int b = 0; dl && b < dl->nlb; ++b) {      /* (named as the pair path names its long class) */
			const bucket* B = &dl->b[b];
			char nm[48];
			const int nlen = B->tailR ? snprintf(nm, sizeof nm, "k_chainq<%d,pairs,%s> x %d strips + 1 of %d", B->R, dl->form[b] == 3 ? "frame" : "int16", B->strips - 1, B->tailR)
			                          : snprintf(nm, sizeof nm, "k_chainq<%d,pairs,%s> x %d strips", B->R, dl->form[b] == 3 ? "frame" : "int16", B->strips);
			if (nlen >= (int)sizeof nm && c->kn.debug) fprintf(stderr, "[ssw_gpu] fill kernel name cut to %d characters\n", (int)sizeof nm - 1);
			note_fill_kernel(c, dl->cells[b], &bestc, nm, dl->form[b] == 3 ? 6.5 : 9.0, B->R, B->strips);
		}
	}
	if (ds && prev_t0 >= 0) {     /* the last chunk */
		const int buf = (chunk_i - 1) & 1;
		int32_t cnt[DB_COUNTERS] = { 0, 0, 0, 0 };
		/* (select mode: the main stream waits for the last selection -- the call's end event then covers it) */
		if ((ds->sel ? ssw_shim_stream_wait_event(c->stream, c->ev_red[buf]) : ssw_shim_event_sync(c->ev_red[buf])) ||
		    ssw_shim_d2h(cnt, d_cnt_s, sizeof cnt, c->stream) || ssw_shim_stream_sync(c->stream)) {
			fail(c, "result download failed: %s", ssw_shim_last_error()); goto done;
		}
		c->tm.n_word += cnt[0]; c->tm.n_byte += cnt[1]; c->tm.db_repeats += cnt[2];
		c->tm.cells += (Q->h_off[nq] - Q->h_off[0]) * (T->h_off[tfirst + tcount] - T->h_off[tfirst]);
		if (!ds->sel) ds->fn_rc = ds->fn(ds->user, tfirst + prev_t0, prev_nt, ds->h_hits[buf]);
	}
	rc = 0;
done:
	free(tk); free(tl_all); free(hres); free(midpairs);
	return rc;
}

/* ------------------------------------------------------------------------------------------------
 * Window passes of one geometry bucket over the jobs in d_list[0 .. cnt): pass 0 locates read_end1 where the fill did not track it
 * (reference src/ssw.c:342-351), pass 1 is the reverse pass that finds the begin position (ssw_align 919-935).  Used by the
 * per-target path (jobs = queries against d_tgt) and by the flagged survivors' phases (survivor_phases: jobs = survivor pairs, vm set).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
	const ssw_gpu_seqs* Q; const ssw_gpu_params* prm;
	const int8_t* d_tgt; int32_t refLen;      /* the target (vm unset), or the longest target (vm set): bounds the window */
	ssw_vmap vm;
	const int8_t* d_mat; int32_t n, maxmat, minmat;
	int fill_form;
	ssw_dres* d_res;
	win_geom g;
} win_in;

/* short-query buckets whose four per-chain profiles would not fit the LDS of a workgroup (alphabets near 32 symbols with many rows per
   lane) take the strip kernel's window mode like the long ones: one profile per wavefront */
static int window_on_strips(const bucket* B, int n) { return B->use_x || ssw_shim_capture_lds_need(B->R, n) > SSW_LDS_LIMIT; }

/* `stream`: where a k_capture launch goes (buckets of a mixed-length batch side by side); the strip kernel's window mode shares
   the context's queue and boundary buffers and always runs on the main stream */
static int window_pass(ssw_gpu_ctx* c, const win_in* wi, const bucket* B, int pass, const int32_t* d_list, int32_t cnt, void* stream)
{
	const ssw_gpu_seqs* Q = wi->Q; const ssw_gpu_params* prm = wi->prm;
	const int32_t n = wi->n, maxmat = wi->maxmat, refLen = wi->refLen;
	const uint32_t gapO2 = (uint32_t)prm->gapO * 0x10001u, gapE2 = (uint32_t)prm->gapE * 0x10001u;
	if (cnt <= 0) return 0;
	const int cap_x = window_on_strips(B, n);
	const int32_t capRmax = wi->g.xrcap < wi->g.xrmax ? wi->g.xrcap : wi->g.xrmax;
	const int32_t capR = B->use_x ? (B->lanes == 64 && B->R > capRmax ? capRmax : B->R) : ((B->P16 + 63) / 64 < capRmax ? (B->P16 + 63) / 64 : capRmax),
	              capL = B->use_x ? B->lanes : wi->g.xlanes;
	if (cap_x) {
		const int32_t hw = halo_for(B->P16, maxmat, prm->gapE);
		const int64_t wcols = (((int64_t)(hw < refLen ? hw : refLen) + 1) + 31) / 16 * 16;
		int64_t per = (int64_t)(c->cm_budget / (size_t)(16 * wcols)); if (per < 1) per = 1;
		for (int32_t q0 = 0; q0 < cnt; q0 += (int32_t)per) {
			const int32_t cnt_q = cnt - q0 < per ? cnt - q0 : (int32_t)per;
			uint32_t* d_bnd = (uint32_t*)ensure(c, &c->bnd, (size_t)(16 * wcols * cnt_q));
			if (!d_bnd) return -1;
			ssw_chainx_args xa; memset(&xa, 0, sizeof xa);
			xa.tgt = wi->d_tgt; xa.refLen = refLen; xa.qcodes = Q->d_codes; xa.qoff = Q->d_off; xa.mat = wi->d_mat; xa.n = n;
			xa.gapO2 = gapO2; xa.gapE2 = gapE2; xa.gapE = prm->gapE; xa.maxmat = maxmat; xa.njobs = cnt_q;
			xa.qlist = d_list + q0; xa.reverse = pass; xa.flag = prm->flag; xa.filters = prm->filters;
			xa.filterd = prm->filterd; xa.res = wi->d_res; xa.bnd = d_bnd; xa.bnd_stride = wcols; xa.lanes = capL; xa.vm = wi->vm;
			/* reverse pass: a window of rows + 25 % almost always contains the whole alignment; the exact
			   halo bound (3x the rows for DNA defaults) is only paid by the alignments that miss */
			int32_t* d_retry = (int32_t*)ensure(c, &c->need, 64);
			if (!d_retry) return -1;
			int32_t missed = 0;
			xa.window_extra = pass ? 64 : -1; xa.retry_count = d_retry;
			xa.banded = pass && capL == 64 && !c->kn.no_band;      /* first try of the reverse pass: the strips walk a diagonal band of the capped window (k_chainq) */
			/* the window passes of the 64-lane chains in the column-frame form too, when the bucket fits its range */
			xa.form = 0; xa.fr_base = 0; xa.fr_kmask = 0;
			if (wi->fill_form != 0 && capL == 64 && !c->kn.window_int16 &&
			    ssw_frame_params(&c->kn, (int64_t)B->P16 * (maxmat > 0 ? maxmat : 0), prm->gapO, prm->gapE, wi->minmat, 64, &xa.fr_base, &xa.fr_kmask)) xa.form = 3;
			const int32_t capS = (B->P16 + capL * capR - 1) / (capL * capR);
			if (ssw_shim_memset(d_retry, 0, sizeof(int32_t), c->stream) ||
			    launch_window_pass(c, capR, capL, capS, &xa, n)) return fail(c, "capture launch failed: %s", ssw_shim_last_error());
			if (pass) {
				if (ssw_shim_d2h(&missed, d_retry, sizeof(int32_t), c->stream) || ssw_shim_stream_sync(c->stream)) return fail(c, "download failed: %s", ssw_shim_last_error());
				if (c->kn.debug) fprintf(stderr, "[ssw_gpu] reverse pass (%s): %d of %d alignments are rerun with the exact window\n", xa.banded ? "capped window, diagonal band" : "capped window", missed, cnt_q);
				if (missed > 0 && xa.banded) {      /* second tier: the alignments whose band did not hold (or could not be proven) take the whole capped window */
					xa.banded = 0;
					if (ssw_shim_memset(d_retry, 0, sizeof(int32_t), c->stream) || launch_window_pass(c, capR, capL, capS, &xa, n)) return fail(c, "capture launch failed: %s", ssw_shim_last_error());
					if (ssw_shim_d2h(&missed, d_retry, sizeof(int32_t), c->stream) || ssw_shim_stream_sync(c->stream)) return fail(c, "download failed: %s", ssw_shim_last_error());
					if (c->kn.debug) fprintf(stderr, "[ssw_gpu] reverse pass (capped window): %d alignments are rerun with the exact window\n", missed);
				}
				if (missed > 0) {
					xa.window_extra = -1; xa.banded = 0;
					if (launch_window_pass(c, capR, capL, capS, &xa, n)) return fail(c, "capture launch failed: %s", ssw_shim_last_error());
				}
			}
		}
		return 0;
	}
	ssw_capture_args ca; memset(&ca, 0, sizeof ca);
	ca.tgt = wi->d_tgt; ca.refLen = refLen; ca.qcodes = Q->d_codes; ca.qoff = Q->d_off; ca.qlist = d_list;
	ca.nq = cnt; ca.mat = wi->d_mat; ca.n = n; ca.gapO2 = gapO2; ca.gapE2 = gapE2; ca.gapE = prm->gapE; ca.maxmat = maxmat;
	ca.reverse = pass; ca.flag = prm->flag; ca.filters = prm->filters; ca.filterd = prm->filterd; ca.res = wi->d_res; ca.vm = wi->vm;
	if (ssw_shim_launch_capture(B->R, &ca, stream ? stream : c->stream)) return fail(c, "capture launch failed: %s", ssw_shim_last_error());
	return 0;
}

/* ------------------------------------------------------------------------------------------------
 * Traceback phase (banded_sw + re-score + band retry, reference src/ssw.c:941-973) over the records d_res[0 .. nslots): the ids in
 * `ids` are offered to the kernels (which skip records without want_cigar), CIGAR slots / resume state are indexed by id.
 * Used by the per-target path (ids = queries against d_tgt) and by the flagged survivors' phases (survivor_phases: ids = survivor pairs, vm set).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
	const ssw_gpu_seqs* Q; const ssw_gpu_params* prm;
	const int8_t* d_tgt; ssw_vmap vm;
	const int8_t* d_mat; int32_t n;
	ssw_dres* d_res; int32_t nslots;
	const int32_t* ids; int32_t nids;      /* host */
	int32_t* d_list;                       /* device scratch for job lists: >= nslots ints (contents are overwritten) */
	int32_t* hneed;                        /* host scratch: nslots ints */
	int list_on_device;                    /* d_list already holds `ids` (the caller's bucket-ordered query list) */
	int32_t maxlen;                        /* longest query */
	int64_t ref_span;                      /* what the target side can add to an alignment's span: min(exact halo of maxlen, longest target) */
} trace_in;
typedef struct { uint32_t* d_cig; int64_t cig_stride; int did_trace; int list_dirty; /* d_list was overwritten */ } trace_out;

/* bytes of one band row of the ONE-wavefront traceback team (ssw_kernels.hip trace_rowbytes / trace_cpt_class with 64 threads), restated for the host: only used to
   tell which alignments round 0's scratch cannot hold anyway (a wrong guess sorts an alignment into the other launch -- never a wrong result) */
static int64_t host_trace_rowbytes1(int64_t band)
{
	const int64_t cells = band * 2 + 3 + 1 + 12, cpt = (band * 2 + 1 + 63) / 64;
	const int64_t C = cpt <= 1 ? 1 : cpt <= 2 ? 2 : cpt <= 4 ? 4 : 0;
	return ((cells + (C > 1 ? cells / C + 3 : 0)) * 4 + 15) & ~(int64_t)15;
}

static int trace_phase(ssw_gpu_ctx* c, const trace_in* ti, trace_out* to)
{
		int64_t cig_stride = 0;
	uint32_t* d_cig = 0;
	int did_trace = 0;
	const ssw_gpu_seqs* Q = ti->Q; const ssw_gpu_params* prm = ti->prm;
	const int8_t* d_tgt = ti->d_tgt; const int8_t* d_mat = ti->d_mat; ssw_dres* d_res = ti->d_res; int32_t* d_qlist = ti->d_list; int32_t* hneed = ti->hneed;
	const int32_t n = ti->n, nq = ti->nslots, maxlen = ti->maxlen;
	to->d_cig = 0; to->cig_stride = 0; to->did_trace = 0; to->list_dirty = 0;
	if (ti->nids > 0) {
		/* one launch over all queries; scratch sized for a band a few doublings wide, grown on demand */
		int64_t span = (int64_t)maxlen + ti->ref_span + 8;
		cig_stride = (span + 3) / 4 * 4;
		d_cig = (uint32_t*)ensure(c, &c->cigar, (size_t)(4 * cig_stride * nq));
		int32_t* d_need = (int32_t*)ensure(c, &c->need, sizeof(int32_t) * 2 * (size_t)nq);
		int32_t* d_resume = (int32_t*)ensure(c, &c->tresume, sizeof(int32_t) * 8 * (size_t)nq);
		if (!d_cig || !d_need || !d_resume) return -1;      /* (the teams' resume state is zeroed before the first team launch) */
		int64_t sstride = ((int64_t)3 * 720 + (int64_t)(2 * 16 + 1) * maxlen * 3 + 64 + 15) / 16 * 16;      /* three rows of a band of 48 (padded: ssw_kernels.hip trace_rowbytes) + 99 direction bytes per row (k_trace: band 16, three bytes per cell) */
		const int wide = n > SSW_MAX_N;      /* the team kernels hold the matrix in 1 KiB of LDS: wider alphabets walk on threads (k_trace reads it through the cache) */
		if (c->kn.trace_wave != 0 && !wide)      /* the team kernels keep one NIBBLE per cell (round 5): a band of 48 is 49 bytes per row */
			sstride = ((int64_t)3 * 720 + (int64_t)49 * maxlen + 64 + 15) / 16 * 16;
		/* long reads: one wavefront per alignment (wide bands, 10^4 rows); short reads: one thread per alignment */
		/* Which kernel walks a band.  Rounds 1-3 gave short reads ONE THREAD per alignment (k_trace) and only reads above 1 kb a TEAM of wavefronts
		   (k_trace_wave: band rows in LDS, a row's cells in parallel, direction bytes packed).  Measured in round 4, the team kernel wins
		   everywhere: a thread's band rows and direction bytes live in HBM scratch and every cell waits for them -- 100 000 x 150-bp
		   tracebacks 17 ms on threads, 6 ms on teams (one wavefront each); 88 000 protein tracebacks 1654 vs 189 ms, 524 000: 11.6 vs 0.64 s;
		   one ssw_align call with flag 2: 1.24 vs 0.96 ms (profiles/round4_dbx.txt, round4_latency.txt).  The thread kernel stays for
		   SSW_GPU_TRACE_WAVE=0 (tests compare the two). */
		const int use_wave0 = wide ? 0 : c->kn.trace_wave >= 0 ? c->kn.trace_wave : 1;
		const int use_wave = wide ? 0 : c->kn.trace_wave >= 0 ? c->kn.trace_wave : 1;      /* rounds after the first */
		const int trace_no_lds = c->kn.trace_no_lds;     /* experiment / test: band rows in HBM scratch instead of LDS */
		const int trace_waves_env = c->kn.trace_waves;   /* experiment / test */
		const int trace_unblocked = c->kn.trace_unblocked;      /* experiment / test: teams with one cell per thread */
		/* round 0: every alignment with a small scratch (band <= 16).  Alignments whose band had to grow report what
		   they needed; later rounds run them in classes of similar need (x4 per class) with 4x headroom. */
		tpend* pend = (tpend*)malloc(sizeof(tpend) * (size_t)nq);     /* key = band that did not fit, need in 4-KiB units, q = query */
		int32_t* lst = (int32_t*)malloc(sizeof(int32_t) * (size_t)nq);
		int32_t* hnb = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)nq);      /* need + band of a round-0 launch */
		int resume_zeroed = 0;
		(void)hneed;
		if (!pend || !lst || !hnb) { free(pend); free(lst); free(hnb); fail(c, "out of host memory%s", ""); return -1; }
		int32_t npend = ti->nids;
		for (int32_t k = 0; k < ti->nids; ++k) { pend[k].key = 0; pend[k].need = 0; pend[k].q = ti->ids[k]; }
		const int64_t full = (int64_t)maxlen + ti->ref_span;
		const int64_t worst = (3 * (2 * full + 8) * 4 + (2 * full + 1) * (int64_t)maxlen * 3 + 64 + 15) / 16 * 16;
		int trace_ok = 1;
		/* Early teams (round 6, EXPERIMENT, off by default: SSW_GPU_TRACE_EARLY=<n> in the hooks build).  banded_sw starts at the band |refLen' - readLen'| + 1
		   (src/ssw.c:941-944): an alignment whose FIRST band already wants more than round 0's scratch (bands above 48) comes back from round 0 at once, untouched --
		   config 4's ~500 unrelated reads, whose teams then walk 10^4 rows five or six times while the device is otherwise nearly idle (VALU busy 0.2).  Those
		   alignments are known from the records before round 0 runs: here their team classes are launched beside round 0 of the narrow ones (a side stream
		   with its own list / scratch / need buffers).  MEASURED on config 4 (profiles/round6_experiments.json): traceback 175 -> 221 ms.  The teams' round is bound
		   by its longest alignment's serial chain, and that chain gets slower when 9 500 issue-bound wavefronts share its compute units (124 -> 168 ms); the handful of
		   narrow alignments that outgrow round 0 then need rounds of their own (38 + 16 ms) instead of riding along with the 497.  The serial order stays. */
		int early = 0, round_first = 0;
		int32_t n_narrow = 0, *lst0 = 0, *hnb0 = 0;
		{
			const int32_t emin = c->kn.trace_early > 0 ? c->kn.trace_early : 2048;
			if (c->kn.trace_early > 0 && use_wave0 && use_wave && !c->kn.trace_diag && ti->nids >= emin &&
			    sstride * (int64_t)ti->nids <= (int64_t)((size_t)32 << 30)) {
				ssw_dres* hr = (ssw_dres*)malloc(sizeof(ssw_dres) * (size_t)nq);
				lst0 = (int32_t*)malloc(sizeof(int32_t) * (size_t)ti->nids); hnb0 = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)ti->nids);
				if (!hr || !lst0 || !hnb0) { free(hr); free(lst0); free(hnb0); free(pend); free(lst); free(hnb); fail(c, "out of host memory%s", ""); return -1; }
				if (ssw_shim_d2h(hr, d_res, sizeof(ssw_dres) * (size_t)nq, c->stream) || ssw_shim_stream_sync(c->stream)) {
					free(hr); free(lst0); free(hnb0); free(pend); free(lst); free(hnb); return fail(c, "result download failed: %s", ssw_shim_last_error());
				}
				int32_t ne = 0;
				for (int32_t k = 0; k < ti->nids; ++k) {
					const int32_t q = ti->ids[k];
					const ssw_dres* r = &hr[q];
					int wide0 = 0; int64_t want = 0, band0 = 0;
					if (r->want_cigar && r->status == 0) {
						const int64_t rl = (int64_t)r->ref_end1 - r->ref_begin1 + 1, ql = (int64_t)r->read_end1 - r->read_begin1 + 1;
						band0 = (rl > ql ? rl - ql : ql - rl) + 1;
						want = 3 * host_trace_rowbytes1(band0) + (band0 + 1) * ql + 16;
						wide0 = want > sstride && band0 < 0x3fffffff;
					}
					if (wide0) { pend[ne].key = (int32_t)band0; pend[ne].need = (int32_t)((want + 4095) >> 12); pend[ne].q = q; ++ne; }
					else lst0[n_narrow++] = q;
				}
				free(hr);
				if (ne >= 8 && n_narrow >= emin / 2) { early = 1; npend = ne; round_first = 1; }
				else { for (int32_t k = 0; k < ti->nids; ++k) { pend[k].key = 0; pend[k].need = 0; pend[k].q = ti->ids[k]; } n_narrow = 0; }
			}
		}
		if (early) {
			void* s0 = c->tstream[5];
			int32_t* d_list0 = (int32_t*)ensure(c, &c->list0, sizeof(int32_t) * (size_t)n_narrow);
			uint8_t* d_scr0 = (uint8_t*)ensure(c, &c->scratch0, (size_t)(sstride * n_narrow));
			int32_t* d_need0 = (int32_t*)ensure(c, &c->need0, sizeof(int32_t) * 2 * (size_t)n_narrow);
			if (!d_list0 || !d_scr0 || !d_need0) { free(lst0); free(hnb0); free(pend); free(lst); free(hnb); return -1; }
			ssw_trace_args ta;
			ta.tgt = d_tgt; ta.qcodes = Q->d_codes; ta.qoff = Q->d_off; ta.qlist = d_list0; ta.nq = n_narrow; ta.mat = d_mat; ta.n = n; ta.vm = ti->vm;
			ta.gapO = prm->gapO; ta.gapE = prm->gapE; ta.res = d_res; ta.scratch = d_scr0; ta.scratch_stride = sstride; ta.soff = 0;
			ta.cigar = d_cig; ta.cigar_stride = cig_stride; ta.need = d_need0; ta.resume = d_resume; ta.unblocked = trace_unblocked; ta.waves = 1;
			ta.lds_bytes = trace_no_lds ? 0 : (int32_t)ssw_shim_trace_lds_need(64, 1);
			resume_zeroed = 1;
			/* (the side stream starts after the window passes and the zeroed resume state on the main stream; the teams below are queued on the main stream
			   and the other side streams right after this event, i.e. ahead of the narrow alignments' wavefronts in the queues) */
			if (ssw_shim_memset(d_resume, 0, sizeof(int32_t) * 8 * (size_t)nq, c->stream) || ssw_shim_event_record(c->ev_db, c->stream) || ssw_shim_stream_wait_event(s0, c->ev_db) ||
			    ssw_shim_h2d(d_list0, lst0, sizeof(int32_t) * (size_t)n_narrow, s0) || ssw_shim_launch_trace_wave(&ta, s0)) {      /* (what it needs comes back in the second phase: a copy into pageable memory would hold the host here until the launch is done) */
				free(lst0); free(hnb0); free(pend); free(lst); free(hnb); return fail(c, "trace launch failed: %s", ssw_shim_last_error());
			}
			to->list_dirty = 1;
			if (c->kn.debug) fprintf(stderr, "[ssw_gpu] %.1f ms: trace, early teams: %d alignments are wide from the start (their classes follow), round 0 of the other %d on a side stream\n", dbg_ms(), npend, n_narrow);
		}
		for (int phase = 0; phase < (early ? 2 : 1) && trace_ok; ++phase) {
		if (phase == 1) {      /* the narrow alignments' round 0 has run beside the teams: whoever outgrew its scratch there goes through the rounds now */
			if (ssw_shim_d2h(hnb0, c->need0.p, sizeof(int32_t) * 2 * (size_t)n_narrow, c->tstream[5]) || ssw_shim_stream_sync(c->tstream[5])) { fail(c, "trace launch failed: %s", ssw_shim_last_error()); trace_ok = 0; break; }
			npend = 0;
			for (int32_t k = 0; k < n_narrow; ++k)
				if (hnb0[k] != 0) {
					if (hnb0[k] < 0) { fail(c, "internal error: CIGAR slot too small%s", ""); trace_ok = 0; break; }
					pend[npend].key = hnb0[n_narrow + k]; pend[npend].need = hnb0[k]; pend[npend].q = lst0[k]; ++npend;
				}
			if (c->kn.debug) fprintf(stderr, "[ssw_gpu] %.1f ms: trace, early teams: round 0 of the narrow alignments done, %d of them pending\n", dbg_ms(), npend);
			did_trace = 1;
			if (!trace_ok) break;
		}
		/* Termination.  An alignment that comes back pending names the band that did not fit and the bytes that band wants; the next round grants
		   at least that (see cap_i below), so the band is walked and the alignment either finishes or reports a band at least twice as wide.
		   banded_sw walks bands <= max(refLen', readLen') only (src/ssw.c:679), the single retry at the full band (945-957) included: after at most
		   log2(span) + 2 rounds nothing is pending.  64 is that bound for any 32-bit span, not a budget -- reaching it would be a bug. */
		for (int round = round_first; round < 64 && npend > 0 && trace_ok; ++round) {
			tpend* nextp = (tpend*)malloc(sizeof(tpend) * (size_t)npend);
			int32_t nnext = 0;
			if (!nextp) { fail(c, "out of host memory%s", ""); trace_ok = 0; break; }
			if (round > 0) qsort(pend, (size_t)npend, sizeof(tpend), tpend_cmp);
			if (round == 0) {
				int64_t per_launch = (int64_t)((size_t)32 << 30) / sstride; if (per_launch < 1) per_launch = 1;
				for (int32_t q0 = 0; q0 < npend && trace_ok; q0 += (int32_t)per_launch) {
					const int32_t cnt_l = npend - q0 < per_launch ? npend - q0 : (int32_t)per_launch;
					for (int32_t k = 0; k < cnt_l; ++k) lst[k] = pend[q0 + k].q;
					uint8_t* d_scr = (uint8_t*)ensure(c, &c->scratch, (size_t)(sstride * cnt_l));
					if (!d_scr) { trace_ok = 0; break; }
					int32_t cnt_row = cnt_l;      /* alignments that go on to the row kernel of this round */
					int list_ready0 = ti->list_on_device && q0 == 0 && cnt_l == npend;
					if (use_wave0 && c->kn.trace_diag) {
						/* (experiment, off by default: SSW_GPU_TRACE_DIAG=1) Narrow bands first: teams of 16 lanes, four alignments per wavefront,
						   bands up to 15 walked by anti-diagonals (k_trace_diag); 72 % of config 4's alignments end there, the others come back
						   with the band that outgrew the team and their state, exactly like an alignment that ran out of scratch, and the row
						   kernel below continues them.  Bit-exact, but one pair of a four-team wavefront costs ~180 instructions: no faster than
						   the row kernel once that one stopped waiting for its stores (profiles/round5_traceback_notes.txt). */
						ssw_trace_args da;
						da.tgt = d_tgt; da.qcodes = Q->d_codes; da.qoff = Q->d_off; da.qlist = d_qlist; da.nq = cnt_l; da.mat = d_mat; da.n = n; da.vm = ti->vm;
						da.gapO = prm->gapO; da.gapE = prm->gapE; da.res = d_res; da.scratch = d_scr; da.scratch_stride = ((int64_t)31 * maxlen + 64 + 15) / 16 * 16; da.soff = 0;
						da.cigar = d_cig; da.cigar_stride = cig_stride; da.need = d_need; da.resume = d_resume; da.unblocked = 0; da.waves = 1; da.lds_bytes = 1024;
						if (!list_ready0) to->list_dirty = 1;
						if (!resume_zeroed) { resume_zeroed = 1; if (ssw_shim_memset(d_resume, 0, sizeof(int32_t) * 8 * (size_t)nq, c->stream)) { fail(c, "memset failed: %s", ssw_shim_last_error()); trace_ok = 0; break; } }
						if ((!list_ready0 && ssw_shim_h2d(d_qlist, lst, sizeof(int32_t) * (size_t)cnt_l, c->stream)) ||
						    ssw_shim_launch_trace_diag(16, &da, c->stream) ||
						    ssw_shim_d2h(hnb, d_need, sizeof(int32_t) * 2 * (size_t)cnt_l, c->stream) ||
						    ssw_shim_stream_sync(c->stream)) { fail(c, "trace launch failed: %s", ssw_shim_last_error()); trace_ok = 0; break; }
						cnt_row = 0;
						for (int32_t k = 0; k < cnt_l; ++k)
							if (hnb[k] != 0) {
								if (hnb[k] < 0) { fail(c, "internal error: CIGAR slot too small%s", ""); trace_ok = 0; break; }
								lst[cnt_row++] = lst[k];
							}
						if (!trace_ok) break;
						if (c->kn.debug) fprintf(stderr, "[ssw_gpu] %.1f ms: trace round 0: %d alignments on 16-lane teams (bands <= 15), %d go on to the row kernel\n", dbg_ms(), cnt_l, cnt_row);
						did_trace = 1;
						list_ready0 = 0;      /* (the list on the device is the whole chunk's: the row kernel takes the compacted one) */
						if (cnt_row == 0) continue;
					}
					ssw_trace_args ta;
					ta.tgt = d_tgt; ta.qcodes = Q->d_codes; ta.qoff = Q->d_off; ta.qlist = d_qlist; ta.nq = cnt_row; ta.mat = d_mat; ta.n = n; ta.vm = ti->vm;
					ta.gapO = prm->gapO; ta.gapE = prm->gapE; ta.res = d_res; ta.scratch = d_scr; ta.scratch_stride = sstride; ta.soff = 0;
					ta.cigar = d_cig; ta.cigar_stride = cig_stride; ta.need = d_need;     /* CIGAR slots are indexed by query */
					ta.resume = d_resume; ta.unblocked = trace_unblocked; ta.waves = 1; ta.lds_bytes = trace_no_lds ? 0 : (int32_t)ssw_shim_trace_lds_need(64, 1);      /* (the round's scratch admits bands up to 48 at the longest read: all of them walk their rows in LDS) */
					/* (the job list is already on the device when the caller's list IS the ids and one launch takes them all; need and band come
					   back in one copy: need[0 .. cnt), band[cnt .. 2 cnt)) */
					const int list_ready = list_ready0;
					if (!list_ready) to->list_dirty = 1;
					if (use_wave0 && !resume_zeroed) { resume_zeroed = 1; if (ssw_shim_memset(d_resume, 0, sizeof(int32_t) * 8 * (size_t)nq, c->stream)) { fail(c, "memset failed: %s", ssw_shim_last_error()); trace_ok = 0; break; } }
					if ((!list_ready && ssw_shim_h2d(d_qlist, lst, sizeof(int32_t) * (size_t)cnt_row, c->stream)) ||
					    (use_wave0 ? ssw_shim_launch_trace_wave(&ta, c->stream) : ssw_shim_launch_trace(&ta, c->stream)) ||
					    ssw_shim_d2h(hnb, d_need, sizeof(int32_t) * 2 * (size_t)cnt_row, c->stream) ||
					    ssw_shim_stream_sync(c->stream)) { fail(c, "trace launch failed: %s", ssw_shim_last_error()); trace_ok = 0; break; }
					for (int32_t k = 0; k < cnt_row; ++k)
						if (hnb[k] != 0) {
							if (hnb[k] < 0) { fail(c, "internal error: CIGAR slot too small%s", ""); trace_ok = 0; break; }
							nextp[nnext].key = hnb[cnt_row + k]; nextp[nnext].need = hnb[k]; nextp[nnext].q = lst[k]; ++nnext;      /* (both kernels report the band that did not fit) */
						}
					if (c->kn.debug) fprintf(stderr, "[ssw_gpu] %.1f ms: trace round 0 (row kernel): %d alignments, scratch %lld B each, %d pending so far\n",
					                                     dbg_ms(), cnt_row, (long long)sstride, nnext);
				}
			} else {
				/* every pending alignment gets a multiple of what it last needed: EIGHT times while that is below 32 MiB (three more band doublings), twice above.  Four
				   times (two doublings) left ONE of config 4's 10 000 alignments pending after the round of the wide bands, and its team then walked 10^4 rows alone on the
				   device: a round of 15.7 ms for one alignment (profiles/round6_traceback_rounds.txt: traceback 172.5 -> 157.9 ms; one-/four-wavefront teams for wider bands
				   than today were measured in the same call and are slower).  The
				   launches of a round -- one per (LDS size, team size) class, split further by the HBM budget -- work on
				   different alignments and different scratch: they are issued on separate streams and run side by side
				   (each is bound by the latency of its longest alignment, not by throughput). */
				int64_t* hoff = (int64_t*)malloc(sizeof(int64_t) * ((size_t)npend * 2 + 2));
				int32_t* hall = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)npend);
				if (!hoff || !hall) { free(hoff); free(hall); free(nextp); fail(c, "out of host memory%s", ""); trace_ok = 0; break; }
				int64_t budget = (int64_t)c->cm_budget;      /* (the same budget as every other phase of the call) */
				{   /* ... but not more than the device has left now (the fill's buffers stay with the context) */
					const int64_t room = (int64_t)c->scratch.cap + (int64_t)(ssw_shim_mem_free_bytes() / 5 * 4);
					if (room > ((int64_t)1 << 30) && budget > room) budget = room;
				}
				for (int32_t k = 0; k < npend; ++k) lst[k] = pend[k].q;
				to->list_dirty = 1;
				if (use_wave && !resume_zeroed) { resume_zeroed = 1; if (ssw_shim_memset(d_resume, 0, sizeof(int32_t) * 8 * (size_t)nq, c->stream)) { fail(c, "memset failed: %s", ssw_shim_last_error()); trace_ok = 0; free(hoff); free(hall); free(nextp); break; } }
				int64_t* d_soff = (int64_t*)ensure(c, &c->goff, sizeof(int64_t) * ((size_t)npend * 2 + 2));
				if (!d_soff || ssw_shim_h2d(d_qlist, lst, sizeof(int32_t) * (size_t)npend, c->stream)) { trace_ok = 0; free(hoff); free(hall); free(nextp); break; }
				for (int32_t b0 = 0; b0 < npend && trace_ok; ) {       /* one batch = what fits the HBM budget at once */
					struct { int32_t g0, g1, waves; int64_t lds, base, soff0; } grp[64];
					int ngrp = 0; int64_t batch_total = 0; int32_t g0 = b0; int64_t soff_at = 0;
					while (g0 < npend && ngrp < 64) {
						int32_t g1 = g0; int64_t total = 0, lds_l = 0; int waves_l = 1;
						hoff[soff_at] = 0;
						while (g1 < npend) {
							const int64_t nb_ = (int64_t)pend[g1].need * 4096;
							int64_t cap_i = (nb_ * (nb_ < ((int64_t)32 << 20) ? c->kn.trace_headroom : 2) + 65536 + 15) / 16 * 16;
							if (cap_i > worst) cap_i = worst > nb_ ? worst : nb_;      /* headroom up to the widest band there can be -- but never less than what was asked for */
							if ((g1 > g0 || ngrp > 0) && batch_total + total + cap_i > budget) break;
							if (use_wave) {
								/* a band row of 2b+1 cells is walked in chunks of 64 cells per wavefront: wide bands get 4 or 16 wavefronts */
								const int32_t b2 = pend[g1].key > (1 << 20) ? (1 << 21) : 2 * pend[g1].key;
								int wv = b2 <= c->kn.trace_w1max ? 1 : b2 <= c->kn.trace_w4max ? 4 : 16;
								/* ... when the round is about LATENCY (config 4: a few hundred wide bands, a compute unit each).  A round of tens of
								   thousands of alignments (the survivors of a protein search: ~300 rows, bands of 50 .. 500) is about THROUGHPUT: a
								   team of 1024 threads on a row of 400 cells leaves 600 of them waiting at two barriers per row, and the device
								   holds 512 such teams at a time.  Then the smallest team whose threads still have <= 4 (one wavefront) or <= 12
								   cells of a row each: 62 114 alignments of the 2048 x 10 000 search 109 -> xx ms (profiles/round5_dbx*.json). */
								if (npend > c->kn.trace_many) wv = b2 <= 254 ? 1 : b2 <= 3070 ? 4 : 16;
								if (trace_waves_env > 0) wv = trace_waves_env;
								/* few LDS classes (16, 64, 80, 128, 160 KiB): only a handful of hardware queues run side by side.  80 KiB (round 6) is HALF a
								   compute unit: a band of 2048 on a 16-wavefront team wants 73 KiB, and in the 128-KiB class config 4's ~490 widest alignments
								   took the 256 compute units one team each, in two rounds; two teams per compute unit make it one (the teams are bound
								   by the latency of a row -- two barriers and a scan --, not by issue: VALU busy 0.28) */
								static const int64_t lds_cls[5] = { 16384, 65536, 81920, 131072, SSW_LDS_LIMIT };
								int64_t l = ssw_shim_trace_lds_need(b2, wv), cls = 131072;
								for (int ci = 0; ci < 5; ++ci) if (l <= lds_cls[ci] && !(ci == 2 && c->kn.trace_no_cls80)) { cls = lds_cls[ci]; break; }      /* (wider than a compute unit's LDS: 128 KiB, rows in HBM scratch as before) */
								if (g1 > g0 && (cls != lds_l || wv != waves_l)) break;     /* pending alignments are sorted by band: classes are contiguous */
								lds_l = cls; waves_l = wv;
							}
							total += cap_i; hoff[soff_at + (g1 - g0) + 1] = total; ++g1;
						}
						if (g1 == g0) break;                               /* budget exhausted: next batch */
						grp[ngrp].g0 = g0; grp[ngrp].g1 = g1; grp[ngrp].waves = waves_l; grp[ngrp].lds = lds_l;
						grp[ngrp].base = batch_total; grp[ngrp].soff0 = soff_at; ++ngrp;
						batch_total += total; soff_at += (g1 - g0) + 1; g0 = g1;
					}
					uint8_t* d_scr = (uint8_t*)ensure(c, &c->scratch, (size_t)batch_total);
					if (!d_scr) { trace_ok = 0; break; }
					if (ssw_shim_h2d(d_soff, hoff, sizeof(int64_t) * (size_t)soff_at, c->stream) || ssw_shim_event_record(c->ev_fill[0], c->stream)) {
						fail(c, "upload failed: %s", ssw_shim_last_error()); trace_ok = 0; break;
					}
					/* widest bands first: they take longest, and only a few hardware queues run side by side */
					int tused[SSW_TSTREAMS];
					for (int sx = 0; sx < SSW_TSTREAMS; ++sx) tused[sx] = 0;
					for (int gx = 0; gx < ngrp && trace_ok; ++gx) {
						const int gi = ngrp - 1 - gx;
						/* (the runtime hands the context's streams to FOUR hardware queues in creation order -- main 1, second 2, side streams 3 4 4 3 2 1 --
						   and launches on one queue run one after the other: the first four launches of a round go to four different queues) */
						static const int side_of[SSW_TSTREAMS] = { 0, 1, 4, 2, 3, 5 };
						void* st = c->stream;
						if (gx > 0) { const int sx = side_of[(gx - 1) % SSW_TSTREAMS]; st = c->tstream[sx]; tused[sx] = 1; }
						const int32_t cnt_l = grp[gi].g1 - grp[gi].g0;
						ssw_trace_args ta;
						ta.tgt = d_tgt; ta.qcodes = Q->d_codes; ta.qoff = Q->d_off; ta.qlist = d_qlist + grp[gi].g0; ta.nq = cnt_l; ta.mat = d_mat; ta.n = n; ta.vm = ti->vm;
						ta.gapO = prm->gapO; ta.gapE = prm->gapE; ta.res = d_res; ta.scratch = d_scr + grp[gi].base; ta.scratch_stride = 0;
						ta.soff = d_soff + grp[gi].soff0;
						ta.cigar = d_cig; ta.cigar_stride = cig_stride; ta.need = d_need + 2 * (int64_t)grp[gi].g0;
						ta.resume = d_resume; ta.unblocked = trace_unblocked; ta.waves = grp[gi].waves; ta.lds_bytes = trace_no_lds ? 0 : (int32_t)grp[gi].lds;
						if (st != c->stream) ssw_shim_stream_wait_event(st, c->ev_fill[0]);
						if (use_wave ? ssw_shim_launch_trace_wave(&ta, st) : ssw_shim_launch_trace(&ta, st)) { fail(c, "trace launch failed: %s", ssw_shim_last_error()); trace_ok = 0; break; }
						if (c->kn.debug) fprintf(stderr, "[ssw_gpu] trace round %d: %d alignments, LDS %lld B x %d waves per alignment, scratch at %lld\n",
						                                     round, cnt_l, (long long)grp[gi].lds, grp[gi].waves, (long long)grp[gi].base);
					}
					for (int sx = 0; sx < SSW_TSTREAMS; ++sx)     /* the main stream continues after every side stream that was handed a launch */
						if (tused[sx] && (ssw_shim_event_record(c->tev[sx], c->tstream[sx]) || ssw_shim_stream_wait_event(c->stream, c->tev[sx]))) {
							fail(c, "stream join failed: %s", ssw_shim_last_error()); trace_ok = 0;
						}
					if (!trace_ok) break;
					if (ssw_shim_d2h(hall + 2 * (int64_t)b0, d_need + 2 * (int64_t)b0, sizeof(int32_t) * 2 * (size_t)(g0 - b0), c->stream) ||
					    ssw_shim_stream_sync(c->stream)) { fail(c, "trace launch failed: %s", ssw_shim_last_error()); trace_ok = 0; break; }
					for (int gi = 0; gi < ngrp && trace_ok; ++gi) {
						const int32_t cnt_l = grp[gi].g1 - grp[gi].g0;
						const int32_t* gneed = hall + 2 * (int64_t)grp[gi].g0; const int32_t* gband = gneed + cnt_l;
						for (int32_t k = 0; k < cnt_l; ++k)
							if (gneed[k] != 0) {
								if (gneed[k] < 0) { fail(c, "internal error: CIGAR slot too small%s", ""); trace_ok = 0; break; }
								nextp[nnext].key = gband[k]; nextp[nnext].need = gneed[k]; nextp[nnext].q = lst[grp[gi].g0 + k]; ++nnext;
							}
					}
					if (c->kn.debug) fprintf(stderr, "[ssw_gpu] %.1f ms: trace round %d: %d launches side by side, %lld B of scratch, %d pending so far\n",
					                                     dbg_ms(), round, ngrp, (long long)batch_total, nnext);
					b0 = g0;
				}
				free(hoff); free(hall);
			}
			did_trace = 1;
			free(pend); pend = nextp; npend = nnext;
		}
		if (early && phase == 0 && trace_ok && npend == 0) {      /* (the list of the second phase is at most the narrow alignments) */
			free(pend);
			pend = (tpend*)malloc(sizeof(tpend) * (size_t)(n_narrow > 0 ? n_narrow : 1));
			if (!pend) { fail(c, "out of host memory%s", ""); trace_ok = 0; }
		}
		}      /* phase */
		if (early) ssw_shim_stream_sync(c->tstream[5]);      /* (also on a failure above: nothing of this call may still be running when its buffers are reused) */
		free(lst0); free(hnb0);
		free(pend); free(lst); free(hnb);
		if (!trace_ok) return -1;
		if (npend > 0) { fail(c, "internal error: traceback scratch negotiation did not converge%s", ""); return -1; }
	}
	if (did_trace && prm->mark_mismatch) {   /* SAM-style CIGARs + edit distance, rewritten on the device */
		const int64_t m_stride = (cig_stride + maxlen + 8 + 3) / 4 * 4;
		uint32_t* d_cig2 = (uint32_t*)ensure(c, &c->cigar2, (size_t)(4 * m_stride * nq));
		if (!d_cig2) return -1;
		ssw_mark_args ma; ma.tgt = d_tgt; ma.qcodes = Q->d_codes; ma.qoff = Q->d_off; ma.nq = nq; ma.res = d_res; ma.cigar = d_cig; ma.vm = ti->vm;
		ma.out = d_cig2; ma.out_stride = m_stride;
		if (ssw_shim_launch_mark(&ma, c->stream)) { fail(c, "mark launch failed: %s", ssw_shim_last_error()); return -1; }
		d_cig = d_cig2;
	}
	to->d_cig = d_cig; to->cig_stride = cig_stride; to->did_trace = did_trace;
	return 0;
}

/* ------------------------------------------------------------------------------------------------
 * The phases of flagged survivors: (query, target) pairs whose forward pass is done and passed the reference's gate (src/ssw.c:916), as
 * ssw_dres records on the device.  One batched reverse pass per geometry bucket (begin positions; read_end1 came with the forward
 * pass), then the traceback over slabs of survivors (a slab = the CIGAR slots that fit half the budget), the completed records to the
 * host and the CIGARs into the call's staging pool.  Used by the flagged database search (dbx_chunk: survivors compacted by k_select)
 * and by the flagged pair lists (pairs_flagged: survivors chosen on the host).  The caller records c->ev_a on the main stream where its
 * locate phase begins (before its own selection / upload).
 * ------------------------------------------------------------------------------------------------ */
typedef struct { bucket b; int64_t first, count; } surv_range;      /* survivors [first, first + count) share the bucket b */
typedef struct {
	const ssw_gpu_seqs* Q; const ssw_gpu_seqs* T; const ssw_gpu_params* prm;
	const int8_t* d_mat; int32_t maxmat, minmat;
	const win_geom* g; int fill_form;
	int32_t maxlen; int64_t maxt;          /* longest query, longest target (window) among the survivors */
	ssw_dres* d_sres; int64_t ns;          /* the survivors' records, ordered by bucket */
	int32_t* d_maps;                       /* four arrays of ns ints: query and target of every survivor (ssw_vmap), the identity list, scratch for the traceback's job lists */
	const ssw_win* d_win;                  /* targets are windows: the device window table (else NULL) */
	const surv_range* rg; int nrg;
	int check_queue;                       /* look at the work queue's error word before returning (chainq_check: one more download and synchronisation) */
} surv_in;
/* hs[0 .. ns): the completed records; pool_off[v]: where survivor v's CIGAR starts in the staging pool (meaningful when it has one) */
static int survivor_phases(ssw_gpu_ctx* c, const surv_in* si, ssw_dres* hs, cigar_stage* st, int64_t* pool_off, double* locate_ms, double* trace_ms)
{
	const ssw_gpu_seqs* Q = si->Q; const ssw_gpu_seqs* T = si->T; const ssw_gpu_params* prm = si->prm;
	const int64_t ns = si->ns;
	int32_t* const d_vq = si->d_maps; int32_t* const d_vt = si->d_maps + ns; int32_t* const d_vl = si->d_maps + 2 * (size_t)ns; int32_t* const d_tl = si->d_maps + 3 * (size_t)ns;
	ssw_vmap vm; vm.vq = d_vq; vm.vt = d_vt; vm.tcodes = T->d_codes; vm.toff = T->d_off; vm.win = si->d_win;
	int32_t* ids = 0; int32_t* hneed = 0; int64_t* goffs = 0;
	int rc = -1;
	/* ---- reverse pass (begin positions), one launch per geometry bucket that has survivors */
	win_in wi; memset(&wi, 0, sizeof wi);
	wi.Q = Q; wi.prm = prm; wi.d_tgt = T->d_codes; wi.refLen = (int32_t)si->maxt; wi.d_mat = si->d_mat; wi.n = prm->n; wi.maxmat = si->maxmat; wi.minmat = si->minmat;
	wi.fill_form = si->fill_form; wi.g = *si->g;
	for (int b = 0; b < si->nrg; ++b) {
		const int64_t f0 = si->rg[b].first;
		if (si->rg[b].count <= 0) continue;
		wi.d_res = si->d_sres + f0; wi.vm = vm; wi.vm.vq = d_vq + f0; wi.vm.vt = d_vt + f0;
		if (window_pass(c, &wi, &si->rg[b].b, 1, d_vl, (int32_t)si->rg[b].count, 0)) goto out;
	}
	ssw_shim_event_record(c->ev_b, c->stream);
	/* ---- traceback over slabs of survivors, CIGARs into the host pool */
	const int32_t halo_max = halo_for((si->maxlen + 15) / 16 * 16, si->maxmat, prm->gapE);
	const int64_t ref_span = halo_max < si->maxt ? halo_max : si->maxt;
	const int64_t slot_bytes = 8 * ((int64_t)si->maxlen + ref_span + 16) + 4 * (int64_t)si->maxlen + 256;
	int64_t slab = (int64_t)(c->cm_budget / 2) / slot_bytes;
	if (slab < 1024) slab = 1024;
	if (c->kn.dbx_slab) slab = c->kn.dbx_slab;
	const int64_t sl = ns < slab ? ns : slab;
	ids = (int32_t*)malloc(sizeof(int32_t) * (size_t)sl); hneed = (int32_t*)malloc(sizeof(int32_t) * (size_t)sl); goffs = (int64_t*)malloc(sizeof(int64_t) * (size_t)sl);
	if (!ids || !hneed || !goffs) { fail(c, "out of host memory%s", ""); goto out; }
	for (int64_t s0 = 0; s0 < ns; s0 += slab) {
		const int32_t cnt = (int32_t)(ns - s0 < slab ? ns - s0 : slab);
		trace_out tro; memset(&tro, 0, sizeof tro);
		if ((prm->flag & 7) != 0) {
			for (int32_t k = 0; k < cnt; ++k) ids[k] = k;
			trace_in tri; memset(&tri, 0, sizeof tri);
			tri.Q = Q; tri.prm = prm; tri.d_tgt = T->d_codes; tri.vm = vm; tri.vm.vq = d_vq + s0; tri.vm.vt = d_vt + s0; tri.d_mat = si->d_mat; tri.n = prm->n;
			tri.d_res = si->d_sres + s0; tri.nslots = cnt; tri.ids = ids; tri.nids = cnt; tri.d_list = d_tl; tri.hneed = hneed; tri.maxlen = si->maxlen; tri.ref_span = ref_span;
			if (trace_phase(c, &tri, &tro)) goto out;
		}
		if (ssw_shim_d2h(hs + s0, si->d_sres + s0, sizeof(ssw_dres) * (size_t)cnt, c->stream) || ssw_shim_stream_sync(c->stream)) { fail(c, "result download failed: %s", ssw_shim_last_error()); goto out; }
		int64_t gwords = 0;
		for (int32_t k = 0; k < cnt; ++k)
			if (hs[s0 + k].status >= 2) { fail(c, "internal error: window pass did not reproduce the forward score%s", ""); goto out; }
		if (cigars_to_stage(c, hs + s0, cnt, si->d_sres + s0, tro.d_cig, st, goffs, 0, &gwords)) goto out;
		if (gwords > 0 && ssw_shim_stream_sync(c->stream)) { fail(c, "CIGAR download failed: %s", ssw_shim_last_error()); goto out; }
		for (int32_t k = 0; k < cnt; ++k) pool_off[s0 + k] = st->n + goffs[k];
		st->n += gwords;
	}
	ssw_shim_event_record(c->ev_c, c->stream);
	if (ssw_shim_stream_sync(c->stream)) { fail(c, "stream sync failed: %s", ssw_shim_last_error()); goto out; }
	if (si->check_queue && chainq_check(c)) goto out;
	*locate_ms += ssw_shim_event_elapsed_ms(c->ev_a, c->ev_b);
	*trace_ms += ssw_shim_event_elapsed_ms(c->ev_b, c->ev_c);
	rc = 0;
out:
	free(ids); free(hneed); free(goffs);
	return rc;
}

static int dbx_chunk(ssw_gpu_ctx* c, dbx_state* dx, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const ssw_gpu_params* prm, const bucket* bk, int nb,
                     const int8_t* d_mat, struct ssw_out_rec* d_out, int32_t tbase, int32_t nt)
{
	const int32_t nk = dx->nqa;
	const int64_t npairs = (int64_t)nk * nt;
	dx->ns = 0;
	if (npairs <= 0) return 0;
	if (npairs > 0x7fffff00) return fail(c, "align_batch: %s", "more than 2^31 (query, target) pairs in one chunk of a flagged database search (lower the scratch budget)");
	const int32_t nblk = (int32_t)((npairs + 255) / 256);
	/* counters: [nblk + 1] block counts / offsets, [nb + 1] first survivor of every bucket; then the buckets' linear start indices */
	const size_t ints = (size_t)nblk + 1 + (size_t)nb + 1;
	int32_t* d_cnt = (int32_t*)ensure(c, &c->scnt, sizeof(int32_t) * ((ints + 1) / 2 * 2) + sizeof(int64_t) * ((size_t)nb + 1));
	int64_t* hlin = (int64_t*)malloc(sizeof(int64_t) * ((size_t)nb + 1));
	int32_t* hfirst = (int32_t*)malloc(sizeof(int32_t) * ((size_t)nb + 2));
	if (!d_cnt || !hlin || !hfirst) { free(hlin); free(hfirst); return d_cnt ? fail(c, "out of host memory%s", "") : -1; }
	int32_t* d_first = d_cnt + nblk + 1;
	int64_t* d_lin = (int64_t*)(d_cnt + (ints + 1) / 2 * 2);
	for (int b = 0; b < nb; ++b) hlin[b] = (int64_t)bk[b].first_q * nt;
	hlin[nb] = npairs;
	int rc = -1;
	surv_range* rg = 0;
	ssw_select_args sa; memset(&sa, 0, sizeof sa);
	sa.out = d_out; sa.order = dx->d_order; sa.nk = nk; sa.nt = nt; sa.tbase = tbase; sa.flag = prm->flag; sa.filters = prm->filters;
	sa.blk = d_cnt; sa.nblk = nblk; sa.bucket_lin = d_lin; sa.nbk = nb; sa.bucket_first = d_first;
	int32_t ns = 0;
	ssw_shim_event_record(c->ev_a, c->stream);
	sa.pass = 0;
	if (ssw_shim_h2d(d_lin, hlin, sizeof(int64_t) * ((size_t)nb + 1), c->stream) || ssw_shim_memset(d_first, 0, sizeof(int32_t) * ((size_t)nb + 1), c->stream) ||
	    ssw_shim_launch_select(&sa, c->stream)) { fail(c, "select launch failed: %s", ssw_shim_last_error()); goto out; }
	sa.pass = 1;
	if (ssw_shim_launch_select(&sa, c->stream) || ssw_shim_d2h(&ns, d_cnt + nblk, sizeof ns, c->stream) || ssw_shim_stream_sync(c->stream)) {
		fail(c, "select launch failed: %s", ssw_shim_last_error()); goto out;
	}
	{
		ssw_dres* d_sres = (ssw_dres*)ensure(c, &c->sres, sizeof(ssw_dres) * (size_t)(ns > 0 ? ns : 1));
		int32_t* d_maps = (int32_t*)ensure(c, &c->svq, sizeof(int32_t) * 4 * (size_t)(ns > 0 ? ns : 1));      /* vq, vt, identity list, traceback job lists */
		if (!d_sres || !d_maps) goto out;
		int32_t* d_vq = d_maps; int32_t* d_vt = d_maps + ns; int32_t* d_vl = d_maps + 2 * (size_t)ns;
		sa.pass = 2; sa.sres = d_sres; sa.svq = d_vq; sa.svt = d_vt; sa.vlist = d_vl; sa.cap = ns;
		if (ssw_shim_launch_select(&sa, c->stream) || ssw_shim_d2h(hfirst, d_first, sizeof(int32_t) * ((size_t)nb + 1), c->stream) || ssw_shim_stream_sync(c->stream)) {
			fail(c, "select launch failed: %s", ssw_shim_last_error()); goto out;
		}
		hfirst[nb] = ns;
		for (int b = nb - 1; b >= 0; --b) if (hlin[b] >= npairs || bk[b].nq == 0) hfirst[b] = hfirst[b + 1];      /* (a start index past the last pair is never visited) */
		dx->survivors += ns;
		if (c->kn.debug) fprintf(stderr, "[ssw_gpu] %.1f ms: flagged database search: targets %d..%d, %d of %lld pairs go on to the reverse pass\n",
		                         dbg_ms(), tbase, tbase + nt - 1, ns, (long long)npairs);
		if (ns == 0) { rc = 0; goto out; }
		if ((size_t)ns > dx->hcap) {
			free(dx->hs); free(dx->hvq); free(dx->hvt); free(dx->hpo);
			dx->hcap = (size_t)ns + (size_t)ns / 4 + 64;
			dx->hs = (ssw_dres*)malloc(sizeof(ssw_dres) * dx->hcap); dx->hvq = (int32_t*)malloc(sizeof(int32_t) * dx->hcap);
			dx->hvt = (int32_t*)malloc(sizeof(int32_t) * dx->hcap); dx->hpo = (int64_t*)malloc(sizeof(int64_t) * dx->hcap);
			if (!dx->hs || !dx->hvq || !dx->hvt || !dx->hpo) { dx->hcap = 0; fail(c, "out of host memory%s", ""); goto out; }
		}
		/* (the survivors' maps for the caller: complete with the first synchronisation of the phases) */
		if (ssw_shim_d2h(dx->hvq, d_vq, sizeof(int32_t) * (size_t)ns, c->stream) || ssw_shim_d2h(dx->hvt, d_vt, sizeof(int32_t) * (size_t)ns, c->stream)) {
			fail(c, "download failed: %s", ssw_shim_last_error()); goto out;
		}
		rg = (surv_range*)malloc(sizeof(surv_range) * (size_t)nb);
		if (!rg) { fail(c, "out of host memory%s", ""); goto out; }
		for (int b = 0; b < nb; ++b) { rg[b].b = bk[b]; rg[b].first = hfirst[b]; rg[b].count = hfirst[b + 1] - hfirst[b]; }
		surv_in si; memset(&si, 0, sizeof si);
		si.Q = Q; si.T = T; si.prm = prm; si.d_mat = d_mat; si.maxmat = dx->maxmat; si.minmat = dx->minmat; si.g = &dx->g; si.fill_form = dx->fill_form;
		si.maxlen = dx->maxlen; si.maxt = dx->maxt; si.d_sres = d_sres; si.d_maps = d_maps; si.ns = ns; si.d_win = 0; si.rg = rg; si.nrg = nb;
		si.check_queue = 0;      /* (this path has never looked at the work queue's error word itself: the context's next chainq_check does) */
		if (survivor_phases(c, &si, dx->hs, dx->stage, dx->hpo, &dx->locate_ms, &dx->trace_ms)) goto out;
		dx->ns = ns;
	}
	rc = 0;
out:
	free(hlin); free(hfirst); free(rg);
	return rc;
}

#define SSW_NOT_STREAMABLE (-3)     /* the fused database-search kernel does not cover this batch: ssw_gpu_search_db takes the generic path */
#define ALIGN16(x) (((size_t)(x) + 15) / 16 * 16)

/* ------------------------------------------------------------------------------------------------
 * ssw_gpu_align_batch: every query against every target of a range.  align_batch_locked (below) is the sequence of phases; what they
 * share lives in two structs.  batch_call: what is fixed for the whole call.  target_plan: what is decided per target.
 * ------------------------------------------------------------------------------------------------ */
typedef struct { ssw_fill_args fa; int R, group; int64_t wgs; } fill_defer;      /* a short-query bucket that joins a multi-bucket grid */
typedef struct {
	const ssw_gpu_seqs* Q; const ssw_gpu_seqs* T; const ssw_gpu_params* prm;
	int32_t tfirst, tcount, nq;
	int32_t n;                             /* letters the kernels address (prm->n, at most SSW_MAX_N_WIDE) */
	int32_t minmat, maxmat, bias;
	int literal;                           /* layout-dependent regime of the reference / wide alphabet: lane-model kernel (k_literal) */
	int32_t maxlen; int64_t maxt;          /* longest query, longest target of the range */
	int may_db, use_dbx;                   /* db_gate: the fused database search may answer the call; ... its flagged form */
	int32_t* order; int32_t nqa;           /* non-empty queries in bucket order */
	ssw_pair* pairs; int32_t npairs_total;
	bucket* bk; int nb;
	uint8_t* qdone;                        /* queries whose records came out of the fused database-search path */
	win_geom geom;
	int8_t* d_mat; ssw_pair* d_pairs; int32_t* d_qlist;      /* the call's small inputs on the device (one upload: batch_header) */
	ssw_dres* d_res;
	uint32_t gapO2, gapE2;
	int fill_form;                         /* tests: SSW_GPU_FILL_FORM=0 (or the older SSW_GPU_FILL_F16=0) keeps the plain int16 form everywhere */
	ssw_dres* hres; int32_t* hneed; int64_t* goffs; cigar_stage pool;      /* host staging: records, traceback needs, CIGAR offsets, CIGARs */
	/* scratch of the phases, sized by the buckets (batch_buckets) */
	keyed* keys; unsigned char* hhdr; bplan* bplans;
	int* border; fill_defer* defer; ssw_reduce_args* rdefer;      /* side-by-side group: buckets by size, deferred fills and reductions */
	/* running sums of the call */
	double fill_ms, locate_ms, trace_ms; int64_t best_fill_cells;
} batch_call;
/* every heap block of the call */
static void batch_call_free(batch_call* bc)
{
	free(bc->order); free(bc->pairs); free(bc->bk); free(bc->qdone); free(bc->hres); free(bc->hneed); free(bc->goffs); free(bc->pool.words);
	free(bc->keys); free(bc->hhdr); free(bc->bplans); free(bc->border); free(bc->defer); free(bc->rdefer);
}

typedef struct {
	int32_t refLen; const int8_t* d_tgt;
	int64_t stride;                        /* columns of a column-maximum row */
	int64_t seg_stride;                    /* rows of the group arrays: 16-byte aligned, padded by >= 4 words (k_reduce_seg loads four groups at a time) */
	bplan* bp;                             /* [nb] (the call's block) */
	int nact, max_chunk, any_dbl, any_chunked;
	int conc;                              /* the buckets run side by side (plan_target) */
	size_t tot_cm, tot_sg, tot_bnd, tot_cand, tot_q, tot_cs;      /* all buckets side by side */
	size_t max_cm, max_sg, max_bnd, max_cand;                      /* one bucket at a time */
	unsigned char *base_cm16, *base_cm8, *base_cmB16, *base_cmB8, *base_sg16, *base_sg8, *base_bnd, *base_cand;      /* plan_alloc */
	int32_t *base_q, *base_cs;
} target_plan;

/* The fused database search (k_filldb) may answer the call: several short targets, scores only -- or flagged (begin positions / CIGARs;
   *use_dbx) with the batched reverse pass and traceback over the pairs that pass the score filter (dbx_chunk, survivor_phases).  The bound on
   the target set dates from the window kernels' 32-bit column indices into the concatenated targets; they take a 64-bit base per job now
   (the pair lists run above 2^31 residues), but this path has not been run there, so the bound stays.  k_filldb takes the column maximum
   of two rows with a 16-bit float max3, valid below 31744: 640 rows x max(mat) <= 49.  Both the half-row class rule (batch_buckets) and
   the database attempt (batch_try_db) ask here. */
static int db_gate(const ssw_gpu_ctx* c, const batch_call* bc, const db_stream* ds, int* use_dbx)
{
	*use_dbx = bc->prm->flag != 0 && !ds && !c->kn.no_dbx && bc->tcount >= 4 && bc->T->total < 0x7fff0000;
	return !c->kn.no_db && (bc->tcount >= 4 || ds) && bc->maxt <= 65000 && bc->maxmat <= 49 && (bc->prm->flag == 0 || *use_dbx);
}

/* bucket the queries by chain geometry, pair neighbours inside a bucket.  Empty queries take no part: the reference gives
   them the empty record (score 0, begins -1; src/ssw.c:900-903), which is what an untouched result record reads as.
   Returns with bc->nqa == 0 (and no buckets) when there is nothing but empty queries. */
static int batch_buckets(ssw_gpu_ctx* c, batch_call* bc, const db_stream* ds)
{
	const ssw_gpu_seqs* Q = bc->Q; const ssw_gpu_seqs* T = bc->T; const ssw_gpu_params* prm = bc->prm;
	const int32_t nq = bc->nq;
	bc->order = (int32_t*)malloc(sizeof(int32_t) * (size_t)nq);
	bc->qdone = (uint8_t*)calloc((size_t)nq, 1);
	bc->pairs = (ssw_pair*)malloc(sizeof(ssw_pair) * ((size_t)nq + 1));
	keyed* const keys = bc->keys = (keyed*)malloc(sizeof(keyed) * (size_t)nq);
	if (!bc->order || !bc->qdone || !bc->pairs || !keys) return fail(c, "out of host memory%s", "");
	int32_t nqa = 0;
	for (int32_t q = 0; q < nq; ++q) {
		int64_t len = Q->h_off[q + 1] - Q->h_off[q];
		if (len > 0x3fffff00) return fail(c, "align_batch: query longer than 2^30 residues%s", "");
		if (len == 0) continue;
		if (len > bc->maxlen) bc->maxlen = (int32_t)len;
		keys[nqa].q = q;
		keys[nqa].key = (int32_t)len; keys[nqa].sub = 0;      /* (the bucket keys follow below, once the strip geometry is known) */
		++nqa;
	}
	bc->nqa = nqa;
	if (nqa == 0) return 0;
	for (int32_t ti = 0; ti < bc->tcount; ++ti) { const int64_t L = T->h_off[bc->tfirst + ti + 1] - T->h_off[bc->tfirst + ti]; if (L > bc->maxt) bc->maxt = L; }
	bc->may_db = db_gate(c, bc, ds, &bc->use_dbx);
	/* bucket keys (the strip geometry decides them: win_bucket_key) */
	win_geom_fill(&bc->geom, &c->kn, bc->n);
	/* Half-row chains (k_fill8): reads with len mod 16 in 1..8 pad to P16 - 8 under 16-bit rules, and eight positions x R8 = 2R - 1 rows are
	   exactly those rows.  A padded-length class takes them (sub 0; short queries of one class otherwise all carry the same sub) only where
	   the kernel can actually run: the batch cannot go to the database-search paths or the lane model, and the frame form fits the class.
	   A class of nothing but such reads is marked as it is.  A class that mixes both kinds of length is SPLIT only when its launches cannot
	   join a side-by-side grid of 16-lane chains anyway -- its column maxima alone are beyond what that needs of the budget, or the hooks
	   build runs the buckets one after the other; a small mixed batch keeps the buckets it always had. */
	const int half_ok = !c->kn.no_fill_half && !c->kn.fill_plain && !bc->literal && !bc->may_db;
	int32_t n_el[SSW_RMAX + 1], n_all[SSW_RMAX + 1];
	memset(n_el, 0, sizeof n_el); memset(n_all, 0, sizeof n_all);
	for (int32_t k = 0; k < nqa; ++k) {
		const int32_t len = keys[k].key;
		keys[k].key = win_bucket_key(&bc->geom, len, &keys[k].sub);
		if (half_ok && keys[k].key <= SSW_RMAX) {
			keys[k].sub = (len - 1) % 16 < 8 && 2 * keys[k].key - 1 <= SSW_R8MAX ? 0 : 1;
			n_all[keys[k].key]++; n_el[keys[k].key] += keys[k].sub == 0;
		}
	}
	if (half_ok) {
		int half_class[SSW_RMAX + 1];
		for (int32_t R = 1; R <= SSW_RMAX; ++R) {
			int32_t hb, hk;
			half_class[R] = n_el[R] > 0 && ssw_frame_params(&c->kn, (int64_t)16 * R * (bc->maxmat > 0 ? bc->maxmat : 0), prm->gapO, prm->gapE, bc->minmat, 8, &hb, &hk);
			if (half_class[R] && n_el[R] < n_all[R]) {
				const int64_t cm_bytes = 8 * ((bc->maxt + 15) / 16 * 16 + 16) * (((int64_t)n_all[R] + 1) / 2);      /* both column-maximum streams of the class */
				half_class[R] = c->kn.serial_buckets || 2 * cm_bytes > (int64_t)c->cm_budget;
			}
		}
		for (int32_t k = 0; k < nqa; ++k) if (keys[k].key <= SSW_RMAX && !half_class[keys[k].key]) keys[k].sub = 1;
	}
	qsort(keys, (size_t)nqa, sizeof(keyed), keyed_cmp);
	for (int32_t i = 0; i < nqa; ) {
		int32_t j = i;
		while (j < nqa && keys[j].key == keys[i].key && (keys[i].key > SSW_RMAX || keys[j].sub == keys[i].sub)) ++j;
		bucket* nbk = (bucket*)realloc(bc->bk, sizeof(bucket) * (size_t)(bc->nb + 1));
		if (!nbk) return fail(c, "out of host memory%s", "");
		bc->bk = nbk;
		bucket b;
		win_bucket_shape(&b, &bc->geom, keys[i].key, keys[j - 1].sub);       /* (sorted by padded length: the last is the longest of the bucket) */
		if (half_ok && keys[i].key <= SSW_RMAX && keys[i].sub == 0) b.half = 2 * b.R - 1;
		b.first_q = i; b.nq = j - i; b.first_pair = bc->npairs_total;
		for (int32_t k = i; k < j; ++k) bc->order[k] = keys[k].q;
		for (int32_t k = i; k < j; k += 2) {
			bc->pairs[bc->npairs_total].qa = bc->order[k];
			bc->pairs[bc->npairs_total].qb = k + 1 < j ? bc->order[k + 1] : -1;
			++bc->npairs_total;
		}
		b.npairs = bc->npairs_total - b.first_pair;
		bc->bk[bc->nb++] = b;
		i = j;
	}
	return 0;
}

/* the call's small inputs -- scoring matrix, query pairs, bucket-ordered query list -- travel in ONE upload (a single-pair ssw_align call is
   bound by the number of dependent operations on its stream, not by their size: profiles/round4_latency.txt) */
static int batch_header(ssw_gpu_ctx* c, batch_call* bc)
{
	const ssw_gpu_params* prm = bc->prm;
	const int32_t n = bc->n;
	const size_t hdr_mat = ((size_t)n * n + 15) / 16 * 16, hdr_pairs = (sizeof(ssw_pair) * (size_t)bc->npairs_total + 15) / 16 * 16;
	const size_t hdr_bytes = hdr_mat + hdr_pairs + sizeof(int32_t) * (size_t)bc->nq;
	unsigned char* d_hdr = (unsigned char*)ensure(c, &c->mat, hdr_bytes);
	bc->d_res = (ssw_dres*)ensure(c, &c->res, sizeof(ssw_dres) * (size_t)bc->nq);
	unsigned char* const hhdr = bc->hhdr = (unsigned char*)malloc(hdr_bytes);      /* host copy of the packed small inputs */
	if (!d_hdr || !bc->d_res) return -1;
	if (!hhdr) return fail(c, "out of host memory%s", "");
	bc->d_mat = (int8_t*)d_hdr;
	bc->d_pairs = (ssw_pair*)(d_hdr + hdr_mat);
	bc->d_qlist = (int32_t*)(d_hdr + hdr_mat + hdr_pairs);
	if (n == prm->n) memcpy(hhdr, prm->mat, (size_t)n * n);
	else for (int32_t r = 0; r < n; ++r) memcpy(hhdr + (size_t)r * n, prm->mat + (size_t)r * prm->n, (size_t)n);      /* the addressable block of a matrix wider than int8 codes */
	memcpy(hhdr + hdr_mat, bc->pairs, sizeof(ssw_pair) * (size_t)bc->npairs_total);
	memcpy(hhdr + hdr_mat + hdr_pairs, bc->order, sizeof(int32_t) * (size_t)bc->nqa);
	ssw_shim_event_record(c->ev_t0, c->stream);
	CALL_TRACE("entry: bucketed, buffers ready");
	if (ssw_shim_h2d(d_hdr, hhdr, hdr_mat + hdr_pairs + sizeof(int32_t) * (size_t)bc->nqa, c->stream)) return fail(c, "upload failed: %s", ssw_shim_last_error());
	return 0;
}

/* the call's timing record and its CIGAR pool, handed to the caller */
static void batch_totals(ssw_gpu_ctx* c, batch_call* bc, uint32_t** cigar_pool, int64_t* cigar_words)
{
	c->tm.total_ms = ssw_shim_event_elapsed_ms(c->ev_t0, c->ev_d); c->tm.fill_ms = bc->fill_ms; c->tm.locate_ms = bc->locate_ms; c->tm.trace_ms = bc->trace_ms;
	c->tm.reduce_ms = c->tm.total_ms - bc->fill_ms - bc->locate_ms - bc->trace_ms;   /* reduction + transfers: everything that is not one of the three timed phases */
	if (c->tm.reduce_ms < 0) c->tm.reduce_ms = 0;
	if (cigar_pool) { *cigar_pool = bc->pool.words; bc->pool.words = 0; }
	if (cigar_words) *cigar_words = bc->pool.n;
}

/* database search: several short targets -> fused kernel for the short-query buckets (scores only, or flagged: db_gate), the strip
   kernel's pair mode for the buckets above them (dbl_class).
   Returns 0: go on with the generic path (for the queries not marked in qdone), 1: the call is answered, SSW_NOT_STREAMABLE, -1: error. */
static int batch_try_db(ssw_gpu_ctx* c, batch_call* bc, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words, db_stream* ds)
{
	const ssw_gpu_seqs* Q = bc->Q;
	const int32_t n = bc->n;
	const int mid_ok = (int64_t)n * 10 * 256 <= 65535;     /* 40 rows per lane: 10 chunks of 256 bytes per residue; n x that must stay a 16-bit offset */
	/* buckets above k_filldb's classes: the long class (dbl_class) takes those whose job fits the scratch rule of the pair path's long class;
	   the others (any_long) stay on the per-target loop */
	dbl_class* dl = 0;
	const int dbl_ok = !bc->literal && bc->may_db && bc->geom.xlanes == 64 && bc->geom.xrmax <= 16;
	int any_short = 0, any_long = 0;
	for (int b = 0; b < bc->nb; ++b) {
		const bucket* B = &bc->bk[b];
		if (!(B->use_x && (B->P16 > 640 || !mid_ok))) { any_short = 1; continue; }
		int32_t lmax = 0;
		for (int32_t k = 0; k < B->nq; ++k) { const int32_t qq = bc->order[B->first_q + k]; const int64_t L = Q->h_off[qq + 1] - Q->h_off[qq]; if (L > lmax) lmax = (int32_t)(L > 0x7fffffff ? 0x7fffffff : L); }
		if (!dbl_ok || lmax > PJ_LONG_MAX || B->R > 16 || plong_job_bytes(bc->maxt, B->strips) > (int64_t)(c->cm_budget / 2)) { any_long = 1; continue; }
		if (!dl) {      /* one block: the record, then room for every bucket of the call (queries of several strips: a bucket per padded length) */
			dl = (dbl_class*)calloc(1, sizeof *dl + (sizeof(bucket) + sizeof(int64_t) + sizeof(int)) * (size_t)bc->nb);
			if (!dl) return fail(c, "out of host memory%s", "");
			dl->cells = (int64_t*)(dl + 1); dl->b = (bucket*)(dl->cells + bc->nb); dl->form = (int*)(dl->b + bc->nb);
		}
		dl->b[dl->nlb++] = *B;
	}
	const int db_ok = !bc->literal && (any_short || dl) && bc->may_db;
	if (ds && (!db_ok || any_long)) { free(dl); return SSW_NOT_STREAMABLE; }
	if (!db_ok) { free(dl); return 0; }
	if (dl) { dl->d_order = bc->d_qlist; dl->maxmat = bc->maxmat; dl->minmat = bc->minmat; }
	dbx_state dxs; memset(&dxs, 0, sizeof dxs);
	if (bc->use_dbx) {
		dxs.order = bc->order; dxs.nqa = bc->nqa; dxs.d_order = bc->d_qlist; dxs.maxmat = bc->maxmat; dxs.minmat = bc->minmat; dxs.maxt = (int32_t)bc->maxt;
		dxs.g = bc->geom; dxs.fill_form = bc->fill_form; dxs.stage = &bc->pool;
	}
	for (int b = 0; b < bc->nb; ++b) if (!bc->bk[b].use_x || (bc->bk[b].P16 <= 640 && mid_ok)) for (int32_t k = 0; k < bc->bk[b].nq; ++k) {
		const int32_t qq = bc->order[bc->bk[b].first_q + k];
		bc->qdone[qq] = 1;
		if (Q->h_off[qq + 1] - Q->h_off[qq] > dxs.maxlen) dxs.maxlen = (int32_t)(Q->h_off[qq + 1] - Q->h_off[qq]);
	}
	for (int b = 0; dl && b < dl->nlb; ++b) for (int32_t k = 0; k < dl->b[b].nq; ++k) {
		const int32_t qq = bc->order[dl->b[b].first_q + k];
		bc->qdone[qq] = 2;
		if (Q->h_off[qq + 1] - Q->h_off[qq] > dxs.maxlen) dxs.maxlen = (int32_t)(Q->h_off[qq + 1] - Q->h_off[qq]);
	}
	for (int32_t q = 0; q < bc->nq; ++q) if (Q->h_off[q + 1] == Q->h_off[q]) bc->qdone[q] = 1;     /* empty queries: empty records, written there */
	int db_rc = align_db(c, Q, bc->T, bc->tfirst, bc->tcount, bc->prm, results, bc->bk, bc->nb, bc->d_pairs, bc->d_mat, bc->bias, (int32_t)bc->maxt, bc->qdone, ds,
	                     bc->use_dbx ? &dxs : 0, dl);
	free(dxs.hs); free(dxs.hvq); free(dxs.hvt); free(dxs.hpo);      /* (the survivors' host copies were patched into the records inside) */
	if (!db_rc && dl && !(ds && ds->fn_rc)) db_rc = chainq_check(c);      /* (the long class ran behind the work queue) */
	free(dl);
	if (db_rc) return -1;
	bc->d_res = (ssw_dres*)ensure(c, &c->res, sizeof(ssw_dres) * (size_t)bc->nq);   /* align_db may have regrown the record buffer */
	if (!bc->d_res) return -1;
	bc->locate_ms += dxs.locate_ms; bc->trace_ms += dxs.trace_ms;
	if (any_long) return 0;
	/* nothing left for the generic path */
	ssw_shim_event_record(c->ev_d, c->stream);
	if (ssw_shim_stream_sync(c->stream)) return fail(c, "stream sync failed: %s", ssw_shim_last_error());
	for (int e = 0; e + 1 < c->nev; e += 2) bc->fill_ms += ssw_shim_event_elapsed_ms(c->ev[e], c->ev[e + 1]);
	batch_totals(c, bc, cigar_pool, cigar_words);
	return 1;
}

/* gapO <= gapE and wide alphabets: the lane-model kernel, both passes */
static int literal_fill(ssw_gpu_ctx* c, batch_call* bc, const target_plan* tp)
{
	const ssw_gpu_seqs* Q = bc->Q; const ssw_gpu_params* prm = bc->prm;
	const int32_t nq = bc->nq, nqa = bc->nqa, refLen = tp->refLen;
	/* scratch per alignment: 4 x [segments][16] int16 + codes + maxColumn (sized for the 16-bit kernel: 8 lanes) */
	const int64_t seg8 = ((int64_t)bc->maxlen + 7) / 8;
	const int64_t lstate = (seg8 * 16 * 2 * 4 + seg8 * 16 + 64 + 15) / 16 * 16;
	const int64_t sstr = (lstate + (int64_t)refLen * 2 + 64 + 15) / 16 * 16;
	int64_t per = (int64_t)(c->cm_budget / (size_t)sstr); if (per < 1) per = 1;
	/* A forward pass that leaves most of the device idle (round 6; the device holds ~50 alignments of this kernel per compute unit) runs BOTH
	   rule sets of every query side by side instead of the 16-bit kernel after the 8-bit one saturated: 2 000 reads x 1 Mb took two kernel
	   lengths on a sixth of the device (45 GCUPS against the reference's 63 on the box's 16 cores, round-5 verdict weak #8). */
	const int spec = prm->score_size == 2 && !c->kn.no_lit_spec && 2 * (int64_t)nqa + 4 <= (int64_t)c->dev_cus * 48 && per >= 2 * (int64_t)nqa + 4;
	int32_t* d_spec = 0;
	if (spec) {
		d_spec = (int32_t*)ensure(c, &c->cand, sizeof(int32_t) * 17 * (size_t)nq);      /* [nq counters][nq x 2 x 8 outcomes] */
		if (!d_spec) return -1;
		if (ssw_shim_memset(d_spec, 0, sizeof(int32_t) * (size_t)nq, c->stream)) return fail(c, "memset failed: %s", ssw_shim_last_error());
	}
	void* e0 = next_event(c); void* e1 = next_event(c);
	ssw_shim_event_record(e0, c->stream);
	for (int pass = 0; pass < (prm->flag != 0 ? 2 : 1); ++pass)
		for (int32_t q0 = 0; q0 < nqa; q0 += (int32_t)per) {      /* (d_qlist holds the nqa NON-EMPTY queries; empty ones keep the zeroed record) */
			const int32_t cnt_q = nqa - q0 < per ? nqa - q0 : (int32_t)per;
			const int64_t regions = spec && pass == 0 ? (((int64_t)cnt_q + 3) & ~(int64_t)3) + cnt_q : cnt_q;      /* (spec: one launch takes all of them, per >= 2 nqa + 4) */
			uint8_t* d_scr = (uint8_t*)ensure(c, &c->scratch, (size_t)(sstr * regions));
			if (!d_scr) return -1;
			ssw_literal_args la;
			la.spec_cnt = spec && pass == 0 ? d_spec : 0; la.spec_out = spec && pass == 0 ? d_spec + nq : 0;
			la.tgt = tp->d_tgt; la.refLen = refLen; la.qcodes = Q->d_codes; la.qoff = Q->d_off; la.qlist = bc->d_qlist + q0; la.nq = cnt_q;
			la.mat = bc->d_mat; la.n = bc->n; la.gapO = prm->gapO; la.gapE = prm->gapE; la.pass = pass; la.maskLen = prm->maskLen; la.bias = bc->bias;
			la.score_size = prm->score_size; la.flag = prm->flag; la.filters = prm->filters; la.filterd = prm->filterd; la.res = bc->d_res;
			la.scratch = d_scr; la.scratch_stride = sstr; la.mc_off = lstate; la.state_bytes = lstate; la.lds_stride = 0;
			if (ssw_shim_launch_literal(&la, c->stream)) return fail(c, "literal launch failed: %s", ssw_shim_last_error());
		}
	ssw_shim_event_record(e1, c->stream);
	c->tm.fill_launches++;
	for (int32_t q = 0; q < nq; ++q) c->tm.fill_cells += (Q->h_off[q + 1] - Q->h_off[q]) * (int64_t)refLen;
	note_fill_kernel(c, c->tm.fill_cells, &bc->best_fill_cells, "k_literal (lane model of the SSE2 kernels)", 0.0, 0, 1);
	return 0;
}

/* Tile geometry, launch size and scratch of one bucket against one target, into *P (its slice offsets are plan_target's).  Pure: reads the
   context's knobs, budget and device sizes; allocates nothing, launches nothing, writes nothing but *P. */
static void plan_bucket(const ssw_gpu_ctx* c, const batch_call* bc, const target_plan* tp, const bucket* B, bplan* P)
{
	const int32_t refLen = tp->refLen;
	const int64_t stride = tp->stride;
	const int32_t Pq = B->P16, halo_full = halo_for(Pq, bc->maxmat, bc->prm->gapE);
	const int use_x = B->use_x;     /* long queries: strip kernel, one job per chain */
	const int gran = use_x ? 1 : 16;     /* k_fill: one workgroup = 16 tiles of one pair */
	int32_t tile, halo, ntiles;
	int64_t want = 1;
	int small_call = 0;
	if ((int64_t)halo_full * 8 * gran < refLen) {
		/* enough chains PER LAUNCH to fill the device several times over, halo overhead <= 1/8.  A launch covers the pairs
		   whose column-maximum arrays fit the budget (8 bytes per column and pair): a 5 Mb target leaves 1600 pairs per
		   launch, which with 16 tiles (one workgroup) per pair would fill little more than half of the device */
		int64_t launch_pairs = use_x ? B->npairs : (int64_t)(c->cm_budget / (size_t)(8 * stride));
		if (launch_pairs < 1) launch_pairs = 1;
		if (launch_pairs > B->npairs) launch_pairs = B->npairs;
		want = (4 * 32768 + B->npairs - 1) / B->npairs;
		if (!use_x && launch_pairs * ((want + 15) / 16) < 6000) want = 16 * ((6000 + launch_pairs - 1) / launch_pairs);   /* >= ~2 rounds of workgroups per launch */
		int64_t maxt = refLen / ((int64_t)halo_full * 8);
		if (want > maxt) want = maxt;
		want = (want + gran - 1) / gran * gran; if (want < gran) want = gran;      /* whole workgroups of 16 chains */
	}
	{
		/* A call that cannot fill the device anyway -- one ssw_align pair, a handful of reads -- is bound by the LATENCY of a chain, tile +
		   halo columns in sequence: then the tiles go down to half the halo (at least 64 columns) as long as all chains of the
		   call still fit the device at once (since round 5: down to an eighth of the halo); the recomputed halos run on compute units that would idle.  One 150-bp read against a
		   10-kb target: 736 steps instead of 10 000 (2.3 -> 0.x ms per ssw_align call, profiles/round4_latency.txt). */
		/* chains a latency-bound call spreads over: for the 16-lane chains TWO workgroups (32 chains, two wavefronts per SIMD) per compute
		   unit -- a step of a lone wavefront is bound by the latency of its dependent instructions (~800 cycles for ~75), a second one hides
		   in it, a third and fourth only share the issue port (measured: 977 workgroups on 256 CUs 0.61 ms per call, 260: 0.57) */
		int64_t slots = use_x ? (int64_t)c->dev_wave_slots : (int64_t)c->dev_cus * (c->device_share > 1 ? 96 : 32);      /* (several caller threads: what the device holds, shared below) */
		if (c->device_share > 1) { slots /= c->device_share; if (slots < 256) slots = 256; }      /* other caller threads' pairs are on the device too */
		const int64_t all_pairs = bc->npairs_total > 0 ? bc->npairs_total : 1;
		if (all_pairs * want < slots && halo_full < refLen) {
			/* (round 5: an eighth of the halo, not half -- a chain's latency is tile + halo steps and the halo is fixed; one 150-bp read against
			   1 Mb: k_fill 240 -> ~185 us of the call's 0.53 ms, profiles/round5_latency_single_pair.json) */
			/* ... for the 16-lane chains of a call that is alone on the device; the strip kernel (two wavefronts per SIMD by its LDS) and
			   calls that share the device with other caller threads keep half a halo: their extra chains would only queue up */
			const int div = !use_x && c->device_share <= 1 ? 8 : 2;
			const int64_t mint = halo_full / div > 64 ? halo_full / div : 64;
			int64_t small = slots / all_pairs;
			if (small > refLen / mint) small = refLen / mint;
			if (small > want) { want = small; small_call = 1; }
		}
	}
	if (want <= 1) { ntiles = 1; tile = (refLen + 15) / 16 * 16; halo = 0; }
	else {
		if (!small_call || want >= gran) want = (want + gran - 1) / gran * gran;      /* (a small call may have fewer tiles than a workgroup has chains: the others stay idle) */
		tile = (int32_t)(((refLen + want - 1) / want + 15) / 16 * 16);
		ntiles = (refLen + tile - 1) / tile; halo = (halo_full + 15) / 16 * 16;     /* (more halo is always exact; multiples of 16 keep the 16-column groups inside one tile) */
		if (ntiles <= 1) { ntiles = 1; tile = (refLen + 15) / 16 * 16; halo = 0; }
	}
	const int64_t maxcols = (((int64_t)tile + halo < refLen ? (int64_t)tile + halo : refLen) + 31) / 16 * 16;
	int64_t per_pair = 8 * stride + (use_x ? 16 * maxcols * ntiles : 0);
	int64_t chunk = (int64_t)(c->cm_budget / (size_t)per_pair);
	/* optional: two column-maximum buffer sets so that k_reduce of chunk i runs on a second stream beside k_fill of chunk i+1 */
	/* measured on MI355X (config 2): overlapping costs more than it saves -- the fill runs at ~100 % VALU issue, so the
	   reduction's waves only take slots from it (2347 ms/step with, 2160 ms without); kept as an opt-in experiment */
	const int dbl = !use_x && chunk < B->npairs && c->kn.overlap;
	/* Pipelined launches (round 6).  A bucket that needs several launches -- its column maxima do not fit the budget at once -- used to
	   run them one after the other on one stream, and every launch ended with a last, partly filled round of workgroups: all
	   workgroups of a launch take the same ~50 ms (config 2), so the device drains for most of a workgroup's duration at two or three
	   workgroups per compute unit instead of seven -- three times per 100 000 reads at a whole-HBM budget, 25 times at 16 GiB (-4 %).
	   Now the launches alternate between the main stream and a second stream, each with its own half of the scratch: the two
	   launches in flight share the compute units, each one's drain and reduction is covered by the other, and launch i + 2 follows
	   the reduction of launch i on its stream.  Same work, same records; only the order in which workgroups reach the compute
	   units changes.  The second stream has the main stream's priority: at the LOWEST priority (the first form; SSW_GPU_PIPE_PRIO=low
	   in the hooks build) its launches only got the slots the main stream's left over, fell behind and ran out the series alone --
	   config 2 on one box, two / four / eight parts at the lowest priority against two at equal priority: 10 073 / 10 211 / 10 282 /
	   10 353 GCUPS under 16 GiB, 10 377 / 10 446 / 10 423 / 10 480 under 64 GiB, 10 398-10 437 / 10 413 / 10 443 / 10 469-10 514 with
	   the whole HBM; more than two parts at equal priority lose again (10 127 under 64 GiB: the streams share hardware queues).
	   profiles/round6_pipeline_parts.txt. */
	const int pipe = !use_x && !dbl && chunk < B->npairs && !c->kn.no_pipe;
	int parts = dbl || pipe ? 2 : 1;
	if (pipe && c->kn.pipe_parts) parts = c->kn.pipe_parts;
	if (parts > 1) chunk = (int64_t)((c->cm_budget / (size_t)parts) / (size_t)per_pair);
	if (chunk < 1) chunk = 1;
	if (chunk > B->npairs) chunk = B->npairs;
	if (!use_x && chunk < B->npairs) {
		/* All workgroups of a launch do the same amount of work, so a launch is as slow as the CU that got one workgroup more
		   than the others: the launches of a bucket get the same number of pairs (not full chunks and a remainder), and that
		   number makes the workgroup count a multiple of the CU count (256 on an unpartitioned MI355X; read from the device).
		   16 tiles per pair left 1600 workgroups per launch on a 5 Mb target: 6 or 7 per CU, 12 % lost. */
		const int64_t bpp = (ntiles + 15) / 16;
		int64_t nl = (B->npairs + chunk - 1) / chunk;
		/* a pipelined series: as many launches on one stream as on the other, so that both reach the end together (5 launches were 3 + 2: the
		   last one ran alone, its drain exposed) */
		if (pipe && parts > 1 && !c->kn.pipe_any_count && nl % parts) nl += parts - nl % parts;
		int64_t even = (B->npairs + nl - 1) / nl;                      /* pairs per launch if all launches are alike */
		const int64_t ncu = c->dev_cus;
		const int64_t unit = (ncu / (bpp > ncu ? ncu : bpp) > 0 ? ncu / (bpp > ncu ? ncu : bpp) : 1) * (B->half ? 2 : 1);      /* pairs that make one workgroup per compute unit (k_fill8: two pairs per workgroup) */
		even = (even + unit - 1) / unit * unit;
		if (even <= chunk) chunk = even;
		else if (chunk >= unit) chunk = chunk / unit * unit;
		if (B->half && (chunk & 1) && chunk > 1) --chunk;      /* whole workgroups of two pairs (a chunk of one pair stays: the second chain is dead) */
	}
	memset(P, 0, sizeof *P);
	P->active = 1;
	P->tile = tile; P->halo = halo; P->ntiles = ntiles; P->maxcols = maxcols; P->chunk = chunk; P->dbl = dbl; P->pipe = pipe && chunk < B->npairs ? parts : 0;
	P->seg = !dbl && !c->kn.no_seg_reduce ;      /* the fill kernels also leave the maxima of 16-column groups, which is all the reduction reads */
	P->cm_bytes = ALIGN16(4 * stride * chunk) * (P->pipe ? P->pipe : 1);      /* (pipe: one set per stream) */
	P->sg_bytes = P->seg ? ALIGN16(4 * tp->seg_stride * chunk) * (P->pipe ? P->pipe : 1) : 0;
	P->bnd_bytes = use_x ? ALIGN16(16 * maxcols * ntiles * chunk) : 0;
	P->cand_bytes = use_x ? ALIGN16(32 * ntiles * chunk) : 0;   /* 2 halves x 4 ints per job */
	if (use_x && B->lanes == 64) { P->q_ints = chainq_queue_ints(chunk * ntiles * B->strips); P->cs_ints = chainq_cands_ints(chunk * ntiles * B->strips); }
}

/* ---- plan: tile geometry and scratch of every geometry bucket against the target (tp->refLen, stride, seg_stride are set), the sums
   over the buckets, and whether the buckets run side by side (allow_conc: the caller has not had that refused yet) */
static void plan_target(const ssw_gpu_ctx* c, const batch_call* bc, target_plan* tp, int allow_conc)
{
	tp->max_chunk = 1; tp->nact = 0;
	tp->tot_cm = tp->tot_sg = tp->tot_bnd = tp->tot_cand = tp->tot_q = tp->tot_cs = 0;
	tp->max_cm = tp->max_sg = tp->max_bnd = tp->max_cand = 0;
	tp->any_dbl = tp->any_chunked = 0;
	for (int b = 0; b < bc->nb; ++b) {
		const bucket* B = &bc->bk[b];
		bplan* P = &tp->bp[b];
		if (bc->qdone[bc->order[B->first_q]]) { memset(P, 0, sizeof *P); continue; }     /* bucket already answered by the database-search path */
		plan_bucket(c, bc, tp, B, P);
		++tp->nact;
		P->cm_off = tp->tot_cm; P->sg_off = tp->tot_sg; P->bnd_off = tp->tot_bnd; P->cand_off = tp->tot_cand; P->q_off = tp->tot_q; P->cs_off = tp->tot_cs;
		tp->tot_cm += P->cm_bytes; tp->tot_sg += P->sg_bytes; tp->tot_bnd += P->bnd_bytes; tp->tot_cand += P->cand_bytes; tp->tot_q += P->q_ints; tp->tot_cs += P->cs_ints;
		if (P->cm_bytes > tp->max_cm) tp->max_cm = P->cm_bytes;
		if (P->sg_bytes > tp->max_sg) tp->max_sg = P->sg_bytes;
		if (P->bnd_bytes > tp->max_bnd) tp->max_bnd = P->bnd_bytes;
		if (P->cand_bytes > tp->max_cand) tp->max_cand = P->cand_bytes;
		if (P->chunk > tp->max_chunk) tp->max_chunk = (int)(P->chunk > 0x7fffffff ? 0x7fffffff : P->chunk);
		tp->any_dbl |= P->dbl; tp->any_chunked |= P->chunk < B->npairs;
	}
	/* Geometry buckets side by side (round 4).  A batch of mixed read lengths -- the reference's own benchmark: 1000 reads of 25-540 bp
	   -- is ~30 buckets with a few pairs each; one after the other on one stream every bucket pays its own partly filled last round
	   of workgroups and the strip kernel's few long jobs leave most of the device idle.  When every bucket is ONE launch and all of
	   them fit the budget together, each gets its own slice of the scratch buffers and its fill + reduction go to one of the side
	   streams; the main stream continues after all of them.  SSW_GPU_SERIAL_BUCKETS=1 keeps the old order (tests compare). */
	tp->conc = tp->nact > 1 && allow_conc && !c->kn.serial_buckets && !c->kn.no_seg_reduce &&     /* (k_reducem reads group maxima only) */
	           !tp->any_dbl && !tp->any_chunked && 2 * tp->tot_cm + 2 * tp->tot_sg + tp->tot_bnd + tp->tot_cand <= c->cm_budget;
	if (!tp->conc) for (int b = 0; b < bc->nb; ++b) { bplan* P = &tp->bp[b]; P->cm_off = P->sg_off = P->bnd_off = P->cand_off = 0; P->q_off = P->cs_off = 0; }
}

/* the scratch of a plan.  Returns 0, or -1: an allocation was refused (c->err says which; plan_retreat) */
static int plan_alloc(ssw_gpu_ctx* c, target_plan* tp)
{
	const int conc = tp->conc;
	tp->base_cm16 = tp->base_cm8 = tp->base_cmB16 = tp->base_cmB8 = tp->base_sg16 = tp->base_sg8 = tp->base_bnd = tp->base_cand = 0;
	tp->base_q = tp->base_cs = 0;
	if (tp->nact == 0) return 0;
	/* (side by side the buffers are the SUM over the buckets: before the budget is cut, the buckets go one after the other -- the maximum) */
	tp->base_cm16 = (unsigned char*)ensure(c, &c->cm16, conc ? tp->tot_cm : tp->max_cm);
	tp->base_cm8 = (unsigned char*)ensure(c, &c->cm8, conc ? tp->tot_cm : tp->max_cm);
	if (!tp->base_cm16 || !tp->base_cm8) return -1;
	tp->base_cmB16 = tp->base_cm16; tp->base_cmB8 = tp->base_cm8;
	if (tp->any_dbl) {
		tp->base_cmB16 = (unsigned char*)ensure(c, &c->cm16b, tp->max_cm); tp->base_cmB8 = (unsigned char*)ensure(c, &c->cm8b, tp->max_cm);
		if (!tp->base_cmB16 || !tp->base_cmB8) return -1;
	}
	if (tp->max_sg) {
		tp->base_sg16 = (unsigned char*)ensure(c, &c->sg16, conc ? tp->tot_sg : tp->max_sg); tp->base_sg8 = (unsigned char*)ensure(c, &c->sg8, conc ? tp->tot_sg : tp->max_sg);
		if (!tp->base_sg16 || !tp->base_sg8) return -1;
	}
	if (tp->max_bnd) {
		tp->base_bnd = (unsigned char*)ensure(c, &c->bnd, conc ? tp->tot_bnd : tp->max_bnd); tp->base_cand = (unsigned char*)ensure(c, &c->cand, conc ? tp->tot_cand : tp->max_cand);
		if (!tp->base_bnd || !tp->base_cand) return -1;
	}
	if (conc && tp->tot_q) {
		tp->base_q = (int32_t*)ensure(c, &c->queue, sizeof(int32_t) * tp->tot_q); tp->base_cs = (int32_t*)ensure(c, &c->cands, sizeof(int32_t) * tp->tot_cs);
		if (!tp->base_q || !tp->base_cs) return -1;
	}
	return 0;
}

/* An allocation that fails although it is within the budget (contexts of ONE process sharing a device; across processes HIP
   over-subscribes silently): what the next plan gives up.  First the side-by-side launches (their buffers are the sum over the buckets),
   then the budget -- to a quarter the first time, a budget that only just fits leaves nothing for the rest of the call, then by halves;
   not when every launch is down to one pair already (a smaller budget cannot shrink them further).  The shim clears HIP's sticky error
   after the failed allocation, so the launches that follow a successful retry do not report it again; ssw_gpu_set_budget starts the
   ladder afresh.  tests/test_emu_pipeline.py runs it.  (ssw_kernels.hip still calls this ladder by its former name, SSW_ALLOC_RETRY.)
   Returns 0 when there is nothing left to give up: c->err keeps the refusal. */
static int plan_retreat(ssw_gpu_ctx* c, int* allow_conc, const target_plan* tp)
{
	if (tp->conc) *allow_conc = 0;
	else if (c->cm_budget > ((size_t)2 << 20) && tp->max_chunk > 1) { c->cm_budget /= c->budget_shrunk ? 2 : 4; c->budget_shrunk = 1; }
	else return 0;
	c->err[0] = 0;
	return 1;
}

/* the scratch of one launch: column maxima under 16-bit and 8-bit rules, and the maxima of their 16-column groups (0: not kept) */
typedef struct { uint32_t *cm16, *cm8, *sg16, *sg8; } fill_bufs;
/* ... of a bucket's plan: its slice when the buckets run side by side, else the whole buffers */
static fill_bufs bucket_bufs(const target_plan* tp, const bplan* P)
{
	fill_bufs fb;
	fb.cm16 = (uint32_t*)(tp->base_cm16 + P->cm_off); fb.cm8 = (uint32_t*)(tp->base_cm8 + P->cm_off);
	fb.sg16 = P->seg ? (uint32_t*)(tp->base_sg16 + P->sg_off) : 0; fb.sg8 = P->seg ? (uint32_t*)(tp->base_sg8 + P->sg_off) : 0;
	return fb;
}

static int32_t* bucket_cand(const ssw_gpu_ctx* c, const target_plan* tp, const bucket* B, const bplan* P)
{
	return B->use_x && !c->kn.no_track ? (int32_t*)(tp->base_cand + P->cand_off) : 0;      /* (no_track, diagnostic: always run the locate pass) */
}

/* arguments of k_fill / k_fill8 / k_fillm for the pairs [p0, p0 + np) of a bucket; `half`: the frame of a chain of 8 positions if it exists.
   Returns whether the half-row chains run. */
static int fill_args_for(const ssw_gpu_ctx* c, const batch_call* bc, const target_plan* tp, const bucket* B, const bplan* P, int32_t p0, int32_t np,
                         const fill_bufs* fb, int half, ssw_fill_args* fa)
{
	const ssw_gpu_params* prm = bc->prm;
	const int64_t top = (int64_t)16 * B->R * (bc->maxmat > 0 ? bc->maxmat : 0);
	fa->tgt = tp->d_tgt; fa->refLen = tp->refLen; fa->qcodes = bc->Q->d_codes; fa->qoff = bc->Q->d_off;
	fa->pairs = bc->d_pairs + B->first_pair + p0; fa->npairs = np; fa->mat = bc->d_mat; fa->n = bc->n;
	fa->gapO2 = bc->gapO2; fa->gapE2 = bc->gapE2; fa->tile = P->tile; fa->halo = P->halo; fa->ntiles = P->ntiles;
	fa->bpp = (P->ntiles + 15) / 16; fa->cm16 = fb->cm16; fa->cm8 = fb->cm8; fa->cm_stride = tp->stride;
	fa->sg16 = fb->sg16; fa->sg8 = fb->sg8; fa->seg_stride = tp->seg_stride;
	/* column-frame form of the recurrence whenever the bucket's scores leave room for the frame offsets below 31744 (no cell of
	   the bucket scores more than its padded length x max(mat)); else plain int16 */
	fa->form = 0; fa->fr_base = 0; fa->fr_kmask = 0; fa->dg = 0;
	if (bc->fill_form != 0 && ssw_frame_params(&c->kn, top, prm->gapO, prm->gapE, bc->minmat, 16, &fa->fr_base, &fa->fr_kmask)) fa->form = 3;
	/* half-row chains: single-bucket launches of the frame form only (the frame of a chain of 8 positions) */
	int32_t hb = 0, hk = 0;
	if (!half || B->use_x || fa->form != 3 || !ssw_frame_params(&c->kn, top, prm->gapO, prm->gapE, bc->minmat, 8, &hb, &hk)) return 0;
	fa->fr_base = hb; fa->fr_kmask = hk;
	fa->dg = fill8_diag_gaps(&c->kn, bc->T, half, bc->n, bc->minmat, prm->gapO, prm->gapE);
	if (fa->dg && c->kn.no_fill_pairs) fa->dg = 2;      /* (test hooks: an instantiation of their build only) */
	return 1;
}

static void reduce_args_for(const ssw_gpu_ctx* c, const batch_call* bc, const target_plan* tp, const bucket* B, const bplan* P, int32_t p0, int32_t np,
                            const fill_bufs* fb, ssw_reduce_args* ra)
{
	const ssw_gpu_params* prm = bc->prm;
	ra->cm16 = fb->cm16; ra->cm8 = fb->cm8; ra->cm_stride = tp->stride; ra->refLen = tp->refLen; ra->pairs = bc->d_pairs + B->first_pair + p0; ra->npairs = np;
	ra->qoff = bc->Q->d_off; ra->maskLen = prm->maskLen; ra->bias = bc->bias; ra->score_size = prm->score_size;
	ra->flag = prm->flag; ra->filters = prm->filters; ra->res = bc->d_res; ra->cand = bucket_cand(c, tp, B, P); ra->tile = P->tile; ra->ntiles = P->ntiles;
	ra->sg16 = fb->sg16; ra->sg8 = fb->sg8; ra->seg_stride = tp->seg_stride;
}

/* The fill of the pairs [p0, p0 + np) of bucket b on stream st: the choice between k_fill, k_fill8, k_chainx and k_chainq, and what the
   call's timing record says about it.  ndefer (side by side): a short-query bucket is not launched, its arguments join the group's
   deferred grids (fill_side_by_side) as bc->defer[(*ndefer)++], and the strip kernel's work queue is the bucket's slice of the group's. */
static int fill_launch(ssw_gpu_ctx* c, batch_call* bc, const target_plan* tp, int b, int32_t p0, int32_t np, const fill_bufs* fb, void* st, int* ndefer)
{
	const bucket* B = &bc->bk[b]; const bplan* P = &tp->bp[b];
	const ssw_gpu_params* prm = bc->prm;
	const int use_x = B->use_x, conc = ndefer != 0;
	const int32_t n = bc->n, refLen = tp->refLen, tile = P->tile, halo = P->halo, ntiles = P->ntiles;
	ssw_fill_args fa;
	const int use_half = fill_args_for(c, bc, tp, B, P, p0, np, fb, B->half && !conc ? B->half : 0, &fa);
	int xform = 0;
	if (use_x) {
		int32_t xfr_base = 0, xfr_kmask = 0;
		if (bc->fill_form != 0 && B->lanes == 64 &&
		    ssw_frame_params(&c->kn, (int64_t)B->P16 * (bc->maxmat > 0 ? bc->maxmat : 0), prm->gapO, prm->gapE, bc->minmat, 64, &xfr_base, &xfr_kmask)) xform = 3;
		ssw_chainx_args xa; memset(&xa, 0, sizeof xa);
		xa.tgt = tp->d_tgt; xa.refLen = refLen; xa.qcodes = bc->Q->d_codes; xa.qoff = bc->Q->d_off; xa.mat = bc->d_mat; xa.n = n;
		xa.gapO2 = bc->gapO2; xa.gapE2 = bc->gapE2; xa.gapE = prm->gapE; xa.maxmat = bc->maxmat; xa.njobs = np * ntiles;
		xa.pairs = fa.pairs; xa.tile = tile; xa.halo = halo; xa.ntiles = ntiles; xa.cm16 = fb->cm16; xa.cm8 = fb->cm8;
		xa.cm_stride = tp->stride; xa.bnd = (uint32_t*)(tp->base_bnd + P->bnd_off); xa.bnd_stride = P->maxcols; xa.cand = bucket_cand(c, tp, B, P); xa.lanes = B->lanes;
		xa.sg16 = fb->sg16; xa.sg8 = fb->sg8; xa.seg_stride = tp->seg_stride;
		if (B->lanes == 64) {     /* strips of all jobs behind one work queue (k_chainq) */
			const int qgrid = chainq_grid(c, B->R, 0, n);
			if (conc ? chainq_setup(c, &xa, B->strips, (int64_t)np * ntiles, qgrid, tp->base_q + P->q_off, tp->base_cs + P->cs_off, st)
			         : chainq_prepare(c, &xa, B->strips, (int64_t)np * ntiles, qgrid)) return -1;
			xa.form = xform; xa.fr_base = xfr_base; xa.fr_kmask = xfr_kmask; xa.tail_R = B->tailR;
			if (c->kn.debug) fprintf(stderr, "[ssw_gpu] chainq fill: R %d (last strip %d), %d jobs x %d strips, %d wavefronts, %s tickets, form %d\n",
			                                     B->R, B->tailR ? B->tailR : B->R, np * ntiles, B->strips, qgrid, xa.whole_jobs ? "job" : "strip", xa.form);
			if (ssw_shim_launch_chainq(B->R, 0, &xa, qgrid, st)) return fail(c, "fill launch failed: %s", ssw_shim_last_error());
			if (c->kn.debug) { const int src = ssw_shim_stream_sync(st); fprintf(stderr, "[ssw_gpu] chainq fill done (sync rc %d: %s)\n", src, src ? ssw_shim_last_error() : "ok"); }
		} else
		if (ssw_shim_launch_chainx(B->R, 0, &xa, st)) return fail(c, "fill launch failed: %s", ssw_shim_last_error());
	} else
	if (conc) {      /* short-query buckets side by side: their workgroups join the grid of their register class (k_fillm) */
		fill_defer* d = &bc->defer[(*ndefer)++];
		d->fa = fa; d->R = B->R; d->wgs = (int64_t)np * fa.bpp; d->group = ssw_shim_fill_class(B->R) * 2 + (fa.form == 3);
	} else
	if (use_half ? ssw_shim_launch_fill8(B->half, &fa, st) : ssw_shim_launch_fill(B->R, &fa, st)) return fail(c, "fill launch failed: %s", ssw_shim_last_error());

	int64_t cols = 0;
	for (int32_t k = 0; k < ntiles; ++k) {
		int64_t lo = (int64_t)k * tile, hi = lo + tile < refLen ? lo + tile : refLen;
		int64_t cf = lo - halo > 0 ? lo - halo : 0;
		cols += hi - cf;
	}
	const int64_t lc = cols * (int64_t)(use_half ? 8 * B->half : B->lanes * (B->tailR ? B->R * (B->strips - 1) + B->tailR : B->R * B->strips)) * 2 * np;
	c->tm.fill_cells += lc;
	char nm[48];
	if (use_half) snprintf(nm, sizeof nm, fa.dg ? "k_fill8<%d,frame> dg" : "k_fill8<%d,frame>", B->half);
	else if (!use_x) snprintf(nm, sizeof nm, "k_fill<%d,%s>", B->R, fa.form == 3 ? "frame" : "int16");
	else if (B->lanes == 64 && B->tailR) snprintf(nm, sizeof nm, "k_chainq<%d,%s> x %d strips + 1 of %d", B->R, xform == 3 ? "frame" : "int16", B->strips - 1, B->tailR);
	else if (B->lanes == 64) snprintf(nm, sizeof nm, "k_chainq<%d,%s> x %d strips", B->R, xform == 3 ? "frame" : "int16", B->strips);
	else snprintf(nm, sizeof nm, "k_chainx<%d,16 lanes> x %d strips", B->R, B->strips);
	note_fill_kernel(c, lc, &bc->best_fill_cells, nm, use_half ? fill8_ops_per_row(B->half, fa.dg) : !use_x ? (fa.form == 3 ? 6.5 : 9.0) : (B->lanes == 64 && xform == 3 ? 6.5 : 9.0), use_half ? B->half : B->R, B->strips);
	return 0;
}

/* One bucket on its own: as many launches of P->chunk pairs as it takes, each followed by its reduction.  Plain: all on the main stream, an
   event pair around every fill.  dbl (opt-in): two buffer sets, the reductions on the second stream beside the next fill.  pipe: the
   launches go round the main stream and the extra one(s), each with its own part of the scratch; one event pair around the series. */
static int fill_bucket_series(ssw_gpu_ctx* c, batch_call* bc, const target_plan* tp, int b)
{
	const bucket* B = &bc->bk[b]; const bplan* P = &tp->bp[b];
	const int dbl = P->dbl;
	const int pipe = P->pipe;      /* the number of parts: 0 (not pipelined), 2 (a hook: up to 8) */
	const fill_bufs A = bucket_bufs(tp, P);
	fill_bufs B2 = A;      /* dbl: the second buffer set */
	if (dbl) { B2.cm16 = (uint32_t*)tp->base_cmB16; B2.cm8 = (uint32_t*)tp->base_cmB8; }
	void *pe0 = 0, *pe1 = 0;
	if (pipe) {
		pe0 = next_event(c); pe1 = next_event(c);
		if (ssw_shim_event_record(pe0, c->stream)) return fail(c, "stream wait failed: %s", ssw_shim_last_error());
		for (int k = 0; k < pipe - 1; ++k) {
			if (!c->pstream[k]) { c->pstream[k] = c->kn.pipe_low_prio ? ssw_shim_stream_create_low() : ssw_shim_stream_create(); c->ev_pipe[k] = ssw_shim_event_create(); }
			if (!c->pstream[k] || !c->ev_pipe[k]) return fail(c, "stream creation failed: %s", ssw_shim_last_error());
			/* (the extra streams start after everything the main stream has queued so far: the call's uploads, the record memset) */
			if (ssw_shim_stream_wait_event(c->pstream[k], pe0)) return fail(c, "stream wait failed: %s", ssw_shim_last_error());
		}
	}
	int launch_i = 0;
	for (int32_t p0 = 0; p0 < B->npairs; p0 += (int32_t)P->chunk, ++launch_i) {
		const int32_t np = B->npairs - p0 < P->chunk ? B->npairs - p0 : (int32_t)P->chunk;
		const int bi = pipe ? launch_i % pipe : dbl ? (launch_i & 1) : 0;
		void* st = c->stream;
		fill_bufs fb = bi ? B2 : A;
		if (pipe) {      /* launch i: part i mod parts of the scratch; parts 1.. on the extra streams (in order on each: launch i + parts follows the reduction of launch i) */
			if (bi) st = c->pstream[bi - 1];
			fb.cm16 = (uint32_t*)((unsigned char*)A.cm16 + (size_t)bi * (P->cm_bytes / (size_t)pipe)); fb.cm8 = (uint32_t*)((unsigned char*)A.cm8 + (size_t)bi * (P->cm_bytes / (size_t)pipe));
			fb.sg16 = P->seg ? (uint32_t*)((unsigned char*)A.sg16 + (size_t)bi * (P->sg_bytes / (size_t)pipe)) : 0;
			fb.sg8 = P->seg ? (uint32_t*)((unsigned char*)A.sg8 + (size_t)bi * (P->sg_bytes / (size_t)pipe)) : 0;
		}
		if (dbl && launch_i >= 2) ssw_shim_stream_wait_event(c->stream, c->ev_red[bi]);    /* the buffer set is free again */
		void *e0 = 0, *e1 = 0;
		if (!pipe) { e0 = next_event(c); e1 = next_event(c); ssw_shim_event_record(e0, st); }
		if (fill_launch(c, bc, tp, b, p0, np, &fb, st, 0)) return -1;
		if (!pipe) ssw_shim_event_record(e1, st);      /* (pipe: one event pair around the whole series, below -- the launches overlap) */
		c->tm.fill_launches++; if (pipe) c->tm.fill_pipelined++;
		ssw_reduce_args ra;
		reduce_args_for(c, bc, tp, B, P, p0, np, &fb, &ra);
		if (dbl) {
			ssw_shim_event_record(c->ev_fill[bi], c->stream);
			ssw_shim_stream_wait_event(c->stream2, c->ev_fill[bi]);
			if (ssw_shim_launch_reduce(&ra, c->stream2)) return fail(c, "reduce launch failed: %s", ssw_shim_last_error());
			ssw_shim_event_record(c->ev_red[bi], c->stream2);
		} else
		if (ssw_shim_launch_reduce(&ra, st)) return fail(c, "reduce launch failed: %s", ssw_shim_last_error());
	}
	if (dbl) {   /* everything later on the main stream sees all records of this bucket */
		ssw_shim_stream_wait_event(c->stream, c->ev_red[0]);
		if (launch_i > 1) ssw_shim_stream_wait_event(c->stream, c->ev_red[1]);
	}
	if (pipe) {   /* the main stream continues after the extra streams' last reductions; the series is timed as one (its reductions included: ~0.1 ms each) */
		for (int k = 0; k < pipe - 1; ++k)
			if (ssw_shim_event_record(c->ev_pipe[k], c->pstream[k]) || ssw_shim_stream_wait_event(c->stream, c->ev_pipe[k])) return fail(c, "stream join failed: %s", ssw_shim_last_error());
		if (ssw_shim_event_record(pe1, c->stream)) return fail(c, "stream join failed: %s", ssw_shim_last_error());
	}
	return 0;
}

/* a side stream's first use in a side-by-side group: it starts after everything the main stream had queued (c->ev_db) */
static int side_stream_join_in(ssw_gpu_ctx* c, int sx, int* side_used)
{
	if (side_used[sx]) return 0;
	side_used[sx] = 1;
	return ssw_shim_stream_wait_event(c->tstream[sx], c->ev_db) ? fail(c, "stream wait failed: %s", ssw_shim_last_error()) : 0;
}
/* ... and the main stream continues after every side stream that was used */
static int side_streams_join_out(ssw_gpu_ctx* c, const int* side_used)
{
	for (int sx = 0; sx < SSW_TSTREAMS; ++sx)
		if (side_used[sx] && (ssw_shim_event_record(c->tev[sx], c->tstream[sx]) || ssw_shim_stream_wait_event(c->stream, c->tev[sx])))
			return fail(c, "stream join failed: %s", ssw_shim_last_error());
	return 0;
}

/* one k_fillm grid per (register class, form) of the ndefer deferred short-query buckets, largest group first, longest chains first */
static int fill_deferred_grids(ssw_gpu_ctx* c, batch_call* bc, int ndefer, int* side_used)
{
	const fill_defer* defer = bc->defer;
	const size_t rec = sizeof(ssw_fill_args);
	unsigned char* htab = (unsigned char*)calloc((rec + 16) * (size_t)ndefer + 64 * 6, 1);
	unsigned char* dtab = (unsigned char*)ensure(c, &c->fmtab, (rec + 16) * (size_t)ndefer + 64 * 6);
	if (!htab) return fail(c, "out of host memory%s", "");
	if (!dtab) { free(htab); return -1; }
	int64_t gw[6] = { 0, 0, 0, 0, 0, 0 };      /* groups by size, largest first */
	for (int i = 0; i < ndefer; ++i) gw[defer[i].group] += defer[i].wgs * defer[i].R;
	int gord[6] = { 0, 1, 2, 3, 4, 5 };
	for (int i = 1; i < 6; ++i) { const int v = gord[i]; int j = i; while (j > 0 && gw[gord[j - 1]] < gw[v]) { gord[j] = gord[j - 1]; --j; } gord[j] = v; }
	size_t at = 0;
	int nside = 0, rc = -1;
	for (int gi_ = 0; gi_ < 6; ++gi_) {
		const int g = gord[gi_];
		int idx[SSW_RMAX + 1], ng = 0;
		for (int i = 0; i < ndefer; ++i) if (defer[i].group == g) idx[ng++] = i;
		if (ng == 0) continue;
		for (int i = 1; i < ng; ++i) { const int v = idx[i]; int j = i; while (j > 0 && defer[idx[j - 1]].R < defer[v].R) { idx[j] = idx[j - 1]; --j; } idx[j] = v; }
		const size_t a0 = at, a1 = a0 + ALIGN16(rec * (size_t)ng), a2 = a1 + ALIGN16(4 * ((size_t)ng + 1));
		int32_t* hfirst = (int32_t*)(htab + a1); int32_t* hR = (int32_t*)(htab + a2);
		int64_t total = 0;
		for (int i = 0; i < ng; ++i) { memcpy(htab + a0 + rec * (size_t)i, &defer[idx[i]].fa, sizeof(ssw_fill_args)); hfirst[i] = (int32_t)total; hR[i] = defer[idx[i]].R; total += defer[idx[i]].wgs; }
		hfirst[ng] = (int32_t)total;
		at = a2 + ALIGN16(4 * (size_t)ng);
		if (total > 0x7fffffff) { fail(c, "internal error: %s", "more than 2^31 workgroups in one multi-bucket fill launch"); goto out; }
		static const int grid_streams[3] = { 0, 1, 4 };      /* three different hardware queues (see fill_side_by_side) */
		const int sx = grid_streams[nside++ % 3];
		void* st = c->tstream[sx];
		if (side_stream_join_in(c, sx, side_used)) goto out;
		ssw_fillm_args ma; ma.sub = (const ssw_fill_args*)(dtab + a0); ma.first_wg = (const int32_t*)(dtab + a1); ma.subR = (const int32_t*)(dtab + a2); ma.nsub = ng;
		if (ssw_shim_h2d(dtab + a0, htab + a0, at - a0, st) || ssw_shim_launch_fillm(&ma, hR, bc->n, g & 1 ? 3 : 0, total, st)) {
			fail(c, "fill launch failed: %s", ssw_shim_last_error()); goto out;
		}
	}
	rc = 0;
out:
	free(htab);
	return rc;
}

/* every bucket's reduction in one grid (k_reducem): one workgroup per pair */
static int reduce_deferred_grid(ssw_gpu_ctx* c, const ssw_reduce_args* rdefer, int nrdefer)
{
	const size_t rec = sizeof(ssw_reduce_args), a1 = ALIGN16(rec * (size_t)nrdefer);
	unsigned char* htab = (unsigned char*)calloc(a1 + 4 * ((size_t)nrdefer + 1) + 16, 1);
	unsigned char* dtab = (unsigned char*)ensure(c, &c->fmtab, a1 + 4 * ((size_t)nrdefer + 1) + 16);
	if (!htab) return fail(c, "out of host memory%s", "");
	if (!dtab) { free(htab); return -1; }
	int32_t* hfirst = (int32_t*)(htab + a1);
	int64_t total = 0;
	for (int i = 0; i < nrdefer; ++i) { memcpy(htab + rec * (size_t)i, &rdefer[i], rec); hfirst[i] = (int32_t)total; total += rdefer[i].npairs; }
	hfirst[nrdefer] = (int32_t)total;
	ssw_reducem_args rm; rm.sub = (const ssw_reduce_args*)dtab; rm.first_wg = (const int32_t*)(dtab + a1); rm.nsub = nrdefer;
	const int bad = ssw_shim_h2d(dtab, htab, a1 + 4 * ((size_t)nrdefer + 1), c->stream) || ssw_shim_launch_reducem(&rm, total, c->stream);
	free(htab);
	return bad ? fail(c, "reduce launch failed: %s", ssw_shim_last_error()) : 0;
}

/* All buckets of a plan side by side (tp->conc): every bucket is one launch in its own slice of the scratch.  The short-query buckets
   first (their grids are the bulk of the work and go to the hardware queues at once), then the strip kernel's launches; the main stream
   continues after all of them with ONE grid of reductions.  The group counts as one launch (its event pair brackets the side streams' work). */
static int fill_side_by_side(ssw_gpu_ctx* c, batch_call* bc, const target_plan* tp)
{
	const bucket* bk = bc->bk; const int nb = bc->nb;
	int* const border = bc->border;
	int side_used[SSW_TSTREAMS]; int ndefer = 0, nrdefer = 0;
	for (int sx = 0; sx < SSW_TSTREAMS; ++sx) side_used[sx] = 0;
	void* ge0 = next_event(c); void* ge1 = next_event(c);
	if (ssw_shim_event_record(ge0, c->stream) || ssw_shim_event_record(c->ev_db, c->stream)) return fail(c, "event record failed: %s", ssw_shim_last_error());
	/* largest bucket first: the side streams are served round-robin, and the device drains the big launches while the small ones fill its gaps */
	for (int i = 0; i < nb; ++i) border[i] = i;
	for (int i = 1; i < nb; ++i) {
		const int v = border[i]; int j = i;
		while (j > 0 && (int64_t)bk[border[j - 1]].npairs * bk[border[j - 1]].P16 < (int64_t)bk[v].npairs * bk[v].P16) { border[j] = border[j - 1]; --j; }
		border[j] = v;
	}
	/* The runtime maps streams onto FOUR hardware queues (seen on ROCm 7.2: the context's eight streams land on queues
	   1 2 3 4 4 3 2 1), and launches that share a queue run one after the other: the strip kernel's few, latency-bound
	   launches all go to ONE side stream, in sequence (together they are shorter than the short-query grids beside them);
	   the multi-bucket grids take three others.  profiles/round4_config6_timeline.txt */
	const int strip_sx = 5;
	if (side_stream_join_in(c, strip_sx, side_used)) return -1;
	for (int pass_x = 0; pass_x < 2; ++pass_x) {
		for (int bi_ = 0; bi_ < nb; ++bi_) {
			const int b = border[bi_];
			const bucket* B = &bk[b]; const bplan* P = &tp->bp[b];
			if (!P->active || (B->use_x != 0) != pass_x) continue;
			const fill_bufs fb = bucket_bufs(tp, P);
			if (fill_launch(c, bc, tp, b, 0, B->npairs, &fb, c->tstream[strip_sx], &ndefer)) return -1;
			reduce_args_for(c, bc, tp, B, P, 0, B->npairs, &fb, &bc->rdefer[nrdefer++]);      /* all reductions of the group as one grid, after the join */
		}
		if (pass_x == 0 && ndefer > 0 && fill_deferred_grids(c, bc, ndefer, side_used)) return -1;
	}
	if (side_streams_join_out(c, side_used)) return -1;
	if (nrdefer > 0 && reduce_deferred_grid(c, bc->rdefer, nrdefer)) return -1;
	ssw_shim_event_record(ge1, c->stream);
	c->tm.fill_launches++;
	return 0;
}

/* window passes of every bucket the generic path answers: read_end1 always (ssw.c:342-351); begin position only when asked for (ssw.c:916) */
static int window_phase(ssw_gpu_ctx* c, const batch_call* bc, const target_plan* tp)
{
	const bucket* bk = bc->bk; const int nb = bc->nb; const int32_t n = bc->n;
	win_in wi; memset(&wi, 0, sizeof wi);
	wi.Q = bc->Q; wi.prm = bc->prm; wi.d_tgt = tp->d_tgt; wi.refLen = tp->refLen; wi.d_mat = bc->d_mat; wi.n = n; wi.maxmat = bc->maxmat; wi.minmat = bc->minmat;
	wi.fill_form = bc->fill_form; wi.d_res = bc->d_res; wi.g = bc->geom;
	/* a batch of many buckets: the k_capture launches (one small, latency-bound grid per bucket) side by side -- a bucket keeps its
	   side stream for both passes (the reverse pass reads what the locate pass wrote) */
	int nwin = 0, wused[SSW_TSTREAMS];
	for (int b = 0; b < nb; ++b) if (!bc->qdone[bc->order[bk[b].first_q]] && !window_on_strips(&bk[b], n)) ++nwin;
	const int fan = nwin > 2 && !c->kn.serial_buckets;
	for (int sx = 0; sx < SSW_TSTREAMS; ++sx) wused[sx] = 0;
	if (fan && ssw_shim_event_record(c->ev_db, c->stream)) return fail(c, "event record failed: %s", ssw_shim_last_error());
	for (int pass = 0; pass < (bc->prm->flag != 0 ? 2 : 1); ++pass)
		for (int b = 0; b < nb; ++b) {
			const bucket* B = &bk[b];
			if (bc->qdone[bc->order[B->first_q]]) continue;
			void* st = 0;
			if (fan && !window_on_strips(B, n)) {
				const int sx = b % SSW_TSTREAMS;
				st = c->tstream[sx];
				if (side_stream_join_in(c, sx, wused)) return -1;
			}
			if (window_pass(c, &wi, B, pass, bc->d_qlist + B->first_q, B->nq, st)) return -1;
		}
	return side_streams_join_out(c, wused);
}

/* traceback (+ SAM-style rewrite) of the alignments whose record asks for a CIGAR; `last`: no further target follows */
static int batch_trace(ssw_gpu_ctx* c, batch_call* bc, const target_plan* tp, int last, trace_out* tro)
{
	const int32_t nq = bc->nq, refLen = tp->refLen;
	const int32_t halo_max = halo_for((bc->maxlen + 15) / 16 * 16, bc->maxmat, bc->prm->gapE);
	trace_in tri; memset(&tri, 0, sizeof tri);
	tri.Q = bc->Q; tri.prm = bc->prm; tri.d_tgt = tp->d_tgt; tri.d_mat = bc->d_mat; tri.n = bc->n; tri.d_res = bc->d_res; tri.nslots = nq;
	tri.ids = bc->order; tri.nids = bc->nqa; tri.d_list = bc->d_qlist; tri.hneed = bc->hneed; tri.maxlen = bc->maxlen; tri.ref_span = halo_max < refLen ? halo_max : refLen;
	tri.list_on_device = 1;
	if (bc->literal) {
		/* gapO <= gapE: the halo argument (every gap base costs at least gapE) does not bound an alignment's reference span -- a gap base can
		   cost gapO, and with gapO = 0 nothing at all: 33 read bases against 346 target bases is a legal answer of the reference.  This regime
		   is not a throughput path: take the spans the window passes actually found (one download) instead of a bound.  CIGAR slots and the
		   traceback's widest band are then exact for this batch. */
		const ssw_dres* hres = bc->hres;
		if (ssw_shim_d2h(bc->hres, bc->d_res, sizeof(ssw_dres) * (size_t)nq, c->stream) || ssw_shim_stream_sync(c->stream)) return fail(c, "result download failed: %s", ssw_shim_last_error());
		int64_t rspan = 1;
		for (int32_t q = 0; q < nq; ++q)
			if (hres[q].want_cigar && hres[q].status == 0 && (int64_t)hres[q].ref_end1 - hres[q].ref_begin1 + 1 > rspan) rspan = (int64_t)hres[q].ref_end1 - hres[q].ref_begin1 + 1;
		tri.ref_span = rspan;
	}
	if (trace_phase(c, &tri, tro)) return -1;
	/* (the traceback may have reordered the query list on the device: the next target's kernels read it in bucket order again) */
	if (tro->list_dirty && !last && ssw_shim_h2d(bc->d_qlist, bc->order, sizeof(int32_t) * (size_t)bc->nqa, c->stream)) return fail(c, "upload failed: %s", ssw_shim_last_error());
	return 0;
}

/* the downloaded records of one target into the caller's array (column ti); CIGARs are named by their offset in the call's pool */
static int records_out(ssw_gpu_ctx* c, const batch_call* bc, int32_t ti, int32_t refLen, ssw_gpu_result* results)
{
	for (int32_t q = 0; q < bc->nq; ++q) {
		const ssw_dres* r = &bc->hres[q];
		ssw_gpu_result* o = &results[(int64_t)q * bc->tcount + ti];
		if (bc->qdone[q]) continue;
		if (r->status >= 2) return fail(c, "internal error: window pass did not reproduce the forward score%s", "");
		o->score1 = (uint16_t)r->score1; o->score2 = (uint16_t)r->score2;
		o->ref_begin1 = r->ref_begin1; o->ref_end1 = r->ref_end1; o->read_begin1 = r->read_begin1; o->read_end1 = r->read_end1;
		o->ref_end2 = r->ref_end2; o->cigarLen = r->cigarLen; o->cigar_off = -1; o->flag = (uint16_t)r->flag; o->status = (uint16_t)r->status;
		o->edit_distance = r->nm;
		if (r->score1 <= 0 && r->status == 0) { o->ref_begin1 = -1; o->read_begin1 = -1; }
		if (r->cigarLen > 0 && r->status == 0) o->cigar_off = bc->pool.n + bc->goffs[q];
		if (r->status == 0 && r->score1 > 0) { if (r->word) c->tm.n_word++; else c->tm.n_byte++; }
		c->tm.cells += (bc->Q->h_off[q + 1] - bc->Q->h_off[q]) * (int64_t)refLen;
	}
	return 0;
}

/* The phases of a batch call, in the order they run.  Per target the fill is either the lane-model kernel (literal_fill) or a plan:
   plan_target decides tiles, launch sizes and -- this is where side by side is chosen -- tp.conc; plan_alloc asks for the scratch; a refusal
   goes to plan_retreat (first no side by side, then a smaller budget) and is planned again, or ends the call when nothing is left to give up. */
static int align_batch_locked(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, int32_t tfirst, int32_t tcount,
                              const ssw_gpu_params* prm, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words, db_stream* ds)
{
	/* ---- 1. check */
	if (!results && !ds) return fail(c, "align_batch: NULL argument%s", "");
	if (check_seqs(c, "align_batch", Q, T, prm)) return -1;
	if (tfirst < 0 || tcount < 0 || tfirst + tcount > T->count) return fail(c, "align_batch: target range out of bounds%s", "");
	if (check_scoring(c, "align_batch", prm)) return -1;
	ssw_shim_set_device(c->device);
	knobs_load(&c->kn);
	if ((Q->count > 1 || tcount > 1 || ds) && ctx_side_streams(c)) return -1;      /* (one pair never leaves the main stream) */
	if (cigar_pool) *cigar_pool = 0;
	if (cigar_words) *cigar_words = 0;
	const int32_t nq = Q->count;
	if (nq == 0 || tcount == 0) return 0;

	/* Alphabets.  The reference takes any int32 n (src/ssw.h:86, ssw.c:826-847).  Up to 32 letters the per-residue score profile of a query
	   lives in LDS (the profile kernels); 33 .. 128 letters -- every value an int8 code can take -- run on the lane-model kernel, which looks
	   its scores up in the MATRIX (n x n bytes of LDS) and is exact in every gap regime, and on the thread traceback, which reads the matrix
	   through the cache: slow (a CPU-class path, like gapO <= gapE), but the reference's answer instead of a refusal.  n > 128: codes are int8,
	   so only the leading 128 x 128 block of the matrix can ever be addressed -- the kernels get that block; the 8-bit bias is still the minimum
	   over the WHOLE matrix, as ssw_init computes it (ssw.c:834-836). */
	batch_call bc; memset(&bc, 0, sizeof bc);
	bc.Q = Q; bc.T = T; bc.prm = prm; bc.tfirst = tfirst; bc.tcount = tcount; bc.nq = nq;
	bc.n = prm->n > SSW_MAX_N_WIDE ? SSW_MAX_N_WIDE : prm->n;
	bc.literal = prm->gapO <= prm->gapE || prm->n > SSW_MAX_N;
	bc.gapO2 = (uint32_t)prm->gapO * 0x10001u; bc.gapE2 = (uint32_t)prm->gapE * 0x10001u;
	bc.fill_form = c->kn.fill_plain ? 0 : -1;
	mat_range(prm, &bc.minmat, &bc.maxmat, &bc.bias);
	int rc = -1;

	/* ---- 2. bucket */
	if (batch_buckets(c, &bc, ds)) goto done;
	if (bc.nqa == 0) {     /* nothing but empty queries */
		rc = ds ? SSW_NOT_STREAMABLE : 0;
		if (!ds) { for (int64_t k = 0; k < (int64_t)nq * tcount; ++k) topk_pad(&results[k]); memset(&c->tm, 0, sizeof c->tm); }
		goto done;
	}
	const int nb1 = bc.nb > 0 ? bc.nb : 1;
	bc.bplans = (bplan*)calloc((size_t)nb1, sizeof(bplan)); bc.border = (int*)malloc(sizeof(int) * (size_t)nb1);
	bc.defer = (fill_defer*)malloc(sizeof(fill_defer) * (size_t)nb1); bc.rdefer = (ssw_reduce_args*)malloc(sizeof(ssw_reduce_args) * (size_t)nb1);
	bc.hres = (ssw_dres*)malloc(sizeof(ssw_dres) * (size_t)nq); bc.hneed = (int32_t*)malloc(sizeof(int32_t) * (size_t)nq); bc.goffs = (int64_t*)malloc(sizeof(int64_t) * (size_t)nq);
	memset(&c->tm, 0, sizeof c->tm);
	c->nev = 0;
	if (!bc.bplans || !bc.border || !bc.defer || !bc.rdefer || !bc.hres || !bc.hneed || !bc.goffs) { fail(c, "out of host memory%s", ""); goto done; }

	/* ---- 3. header upload; 4. the database path, where it answers (part of) the call */
	if (batch_header(c, &bc)) goto done;
	rc = batch_try_db(c, &bc, results, cigar_pool, cigar_words, ds);
	if (rc != 0) { if (rc == 1) rc = 0; goto done; }
	rc = -1;

	/* ---- 5. per target */
	for (int32_t ti = 0; ti < tcount; ++ti) {
		const int64_t refLen64 = T->h_off[tfirst + ti + 1] - T->h_off[tfirst + ti];
		if (refLen64 > 0x7fffff00) { fail(c, "align_batch: target longer than 2^31 is not supported%s", ""); goto done; }
		const int32_t refLen = (int32_t)refLen64;
		const int ev_first = c->nev;
		target_plan tp; memset(&tp, 0, sizeof tp);
		tp.refLen = refLen; tp.d_tgt = T->d_codes + T->h_off[tfirst + ti]; tp.bp = bc.bplans;
		tp.stride = ((int64_t)refLen + 15) / 16 * 16 + 16; tp.seg_stride = (tp.stride / 16 + 4 + 3) / 4 * 4;
		/* (every non-empty query's record is written whole by the reduction; only empty queries, queries answered elsewhere and an EMPTY
		   target -- no kernel runs at all: the reference's score-0 record, src/ssw.c:900-903 -- rely on zeroes) */
		if ((bc.nqa != nq || tcount > 1 || refLen == 0) && ssw_shim_memset(bc.d_res, 0, sizeof(ssw_dres) * (size_t)nq, c->stream)) { fail(c, "memset failed: %s", ssw_shim_last_error()); goto done; }

		if (refLen > 0 && bc.literal) { if (literal_fill(c, &bc, &tp)) goto done; }
		else if (refLen > 0) {
			int allow_conc = 1;      /* (per target: the next target may try side by side again) */
			for (;;) {
				plan_target(c, &bc, &tp, allow_conc);
				if (!plan_alloc(c, &tp)) break;
				if (!plan_retreat(c, &allow_conc, &tp)) goto done;
			}
			if (tp.conc) { if (fill_side_by_side(c, &bc, &tp)) goto done; }
			else for (int b = 0; b < bc.nb; ++b) if (tp.bp[b].active && fill_bucket_series(c, &bc, &tp, b)) goto done;
		}
		ssw_shim_event_record(c->ev_a, c->stream);
		CALL_TRACE("fill + reduction enqueued");

		if (refLen > 0 && !bc.literal && window_phase(c, &bc, &tp)) goto done;
		ssw_shim_event_record(c->ev_b, c->stream);
		CALL_TRACE("window passes enqueued");

		trace_out tro; memset(&tro, 0, sizeof tro);
		if ((prm->flag & 7) != 0 && refLen > 0 && batch_trace(c, &bc, &tp, ti + 1 == tcount, &tro)) goto done;
		ssw_shim_event_record(c->ev_c, c->stream);
		CALL_TRACE("traceback enqueued / negotiated");

		if (chainq_check(c)) goto done;
		if (ssw_shim_d2h(bc.hres, bc.d_res, sizeof(ssw_dres) * (size_t)nq, c->stream) || ssw_shim_stream_sync(c->stream)) {
			fail(c, "result download failed: %s", ssw_shim_last_error()); goto done;
		}
		int64_t gwords = 0;
		if (cigars_to_stage(c, bc.hres, nq, bc.d_res, tro.d_cig, &bc.pool, bc.goffs, nq <= 4, &gwords)) goto done;
		if (records_out(c, &bc, ti, refLen, results)) goto done;
		bc.pool.n += gwords;
		ssw_shim_event_record(c->ev_d, c->stream);
		CALL_TRACE("results + CIGARs on the host");
		if (ssw_shim_stream_sync(c->stream)) { fail(c, "stream sync failed: %s", ssw_shim_last_error()); goto done; }
		for (int e = ev_first; e + 1 < c->nev; e += 2) bc.fill_ms += ssw_shim_event_elapsed_ms(c->ev[e], c->ev[e + 1]);
		bc.locate_ms += ssw_shim_event_elapsed_ms(c->ev_a, c->ev_b);
		bc.trace_ms += ssw_shim_event_elapsed_ms(c->ev_b, c->ev_c);
	}

	/* ---- 6. totals */
	batch_totals(c, &bc, cigar_pool, cigar_words);
	rc = 0;
done:
	/* a failed call may have launches queued on the side streams: nothing of it may still run when the caller frees or reuses the buffers
	   (SSW_NOT_STREAMABLE is no failure: batch_try_db returns it before anything goes to a side stream, and the caller goes on) */
	if (rc != 0 && rc != SSW_NOT_STREAMABLE) ctx_drain(c);
	batch_call_free(&bc);
	return rc;
}

int ssw_gpu_align_batch(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, int32_t tfirst, int32_t tcount,
                        const ssw_gpu_params* prm, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!c) return fail(0, "align_batch: NULL context%s", "");
	if (ctx_enter(c, cigar_pool, cigar_words)) return SSW_GPU_BUSY;
	return ctx_leave(c, align_batch_locked(c, Q, T, tfirst, tcount, prm, results, cigar_pool, cigar_words, 0));
}

int ssw_gpu_search_db(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const ssw_gpu_params* prm,
                      int32_t targets_per_chunk, ssw_gpu_hits_fn fn, void* user)
{
	if (!c) return fail(0, "search_db: NULL context%s", "");
	if (!Q || !T || !prm || !fn || !prm->mat) return fail(c, "search_db: NULL argument%s", "");
	if (Q->ctx != c || T->ctx != c) return fail(c, "search_db: sequences belong to another context%s", "");
	if (prm->flag != 0) return fail(c, "search_db: scores and end positions only (flag must be 0)%s", "");
	if (ctx_enter(c, 0, 0)) return SSW_GPU_BUSY;      /* (no pool outputs) */
	ssw_shim_set_device(c->device);
	const int32_t nq = Q->count, nt_all = T->count;
	int rc = 0;
	if (nq > 0 && nt_all > 0) {
		int64_t chunk = targets_per_chunk > 0 ? targets_per_chunk : 2048;
		/* two device + two page-locked host buffers of nq x chunk compact records: keep each below 2 GiB */
		while (chunk > 16 && (int64_t)nq * chunk * (int64_t)sizeof(ssw_gpu_hit) > ((int64_t)2 << 30)) chunk /= 2;
		if (chunk > nt_all) chunk = nt_all;
		const size_t bytes = sizeof(ssw_gpu_hit) * (size_t)nq * (size_t)chunk;
		db_stream ds; memset(&ds, 0, sizeof ds);
		ds.chunk = (int32_t)chunk; ds.fn = fn; ds.user = user; ds.cnt_off = bytes;
		if (c->hits_cap < bytes) {      /* (page-locking gigabytes takes of the order of a second: the buffers stay with the context) */
			for (int i = 0; i < 2; ++i) { ssw_shim_free(c->hits_d[i]); ssw_shim_host_free(c->hits_h[i]); c->hits_d[i] = 0; c->hits_h[i] = 0; }
			c->hits_cap = 0;
			for (int i = 0; i < 2; ++i) { c->hits_d[i] = ssw_shim_malloc(bytes); c->hits_h[i] = ssw_shim_host_alloc(bytes + 64); }   /* + the counter snapshot */
			if (c->hits_d[0] && c->hits_d[1] && c->hits_h[0] && c->hits_h[1]) c->hits_cap = bytes;
		}
		for (int i = 0; i < 2; ++i) { ds.d_hits[i] = (struct ssw_hit_rec*)c->hits_d[i]; ds.h_hits[i] = (ssw_gpu_hit*)c->hits_h[i]; }
		if (c->hits_cap < bytes) rc = fail(c, "search_db: buffer allocation failed: %s", ssw_shim_last_error());
		else rc = align_batch_locked(c, Q, T, 0, nt_all, prm, 0, 0, 0, &ds);
		if (rc == SSW_NOT_STREAMABLE) {
			/* generic path (matrices with entries above 49, gapO <= gapE, wide alphabets, targets over 65 000 columns, a long query whose job
			   does not fit the scratch rule of the long class): full records per chunk, converted on the host -- same values, no overlap */
			ssw_gpu_result* full = (ssw_gpu_result*)ssw_shim_host_alloc(sizeof(ssw_gpu_result) * (size_t)nq * (size_t)chunk);
			rc = full ? 0 : fail(c, "search_db: buffer allocation failed: %s", ssw_shim_last_error());
			for (int32_t t0 = 0; rc == 0 && t0 < nt_all; t0 += (int32_t)chunk) {
				const int32_t nt = nt_all - t0 < chunk ? nt_all - t0 : (int32_t)chunk;
				rc = align_batch_locked(c, Q, T, t0, nt, prm, full, 0, 0, 0);
				if (rc) break;
				for (int64_t k = 0; k < (int64_t)nq * nt; ++k) {
					ssw_gpu_hit* h = &ds.h_hits[0][k]; const ssw_gpu_result* r = &full[k];
					h->score1 = r->score1; h->score2 = r->score2; h->ref_end1 = r->ref_end1; h->read_end1 = r->read_end1;
					h->ref_end2 = r->status == 1 ? -2 : r->ref_end2;
				}
				ds.fn_rc = fn(user, t0, nt, ds.h_hits[0]);
				if (ds.fn_rc) break;
			}
			ssw_shim_host_free(full);
		}
		if (rc == 0 && ds.fn_rc) rc = ds.fn_rc;
		ssw_shim_stream_sync(c->stream); ssw_shim_stream_sync(c->stream2);
	}
	return ctx_leave(c, rc);
}

/* ------------------------------------------------------------------------------------------------
 * Explicit pair lists (ssw_gpu_align_pairs): results[i] = the record of (query qidx[i], target tidx[i]) -- a mapper's
 * "for each read: Align(read, its window)" loop as one call.
 *   envelope (gapO > gapE, n <= 32, max(mat) <= 49, queries 1..640 residues, targets 1..65000 columns -- the fused
 *   database search's gates): k_fillpairs, jobs of two pairs that share the row class R = ceil(len / 16), one chain per job,
 *   final records in one launch per R (and per chunk of the scratch budget).  Planning is a counting sort by (R, target-length
 *   class): O(npairs), no comparison sort.
 *   long class (gapO > gapE, n <= 32, queries 769..65535 residues, targets 1..65000 columns, a job's scratch within half the budget;
 *   no max(mat) gate): the strip kernel's pair mode, k_chainq<R,pairs,form> behind its work queue + k_reduce_pairs, one series of
 *   launches per bucket of win_bucket_key; its jobs continue the numbering of k_fillpairs' jobs, records in the same arrays.
 *   flag != 0: the pairs of both classes that pass the score gate then go through one batched reverse pass and traceback (pairs_flagged);
 *   everything else (empty sequences, queries of 641..768 residues, longer targets, gapO <= gapE, wide alphabets, large scores): one internal
 *   batch per distinct target over the subset of its queries, gathered into a temporary set on the device (k_seqgather) --
 *   exact, and slow: a batch call per target.
 * ------------------------------------------------------------------------------------------------ */
/* where the target of pair i comes from: the whole target tidx[i] (ssw_gpu_align_pairs: tbeg NULL), or its columns [tbeg[i], tbeg[i] +
   tlen[i]) (ssw_gpu_align_windows).  The kernels name a pair's target by ps_tid: the target index, or -- windows -- the pair's own entry of
   the device window table d_win. */
typedef struct { const int32_t* tidx; const int64_t* tbeg; const int32_t* tlen; const ssw_win* d_win; const char* who; } pair_src;
static inline int64_t ps_tlen(const pair_src* s, const ssw_gpu_seqs* T, int64_t i) { return s->tbeg ? (int64_t)s->tlen[i] : T->h_off[s->tidx[i] + 1] - T->h_off[s->tidx[i]]; }
static inline int32_t ps_tid(const pair_src* s, int64_t i) { return s->tbeg ? (int32_t)i : s->tidx[i]; }

#define PJ_TCLS 2048      /* target-length classes of the planner: 32 columns each (65000 columns: 2031 classes) */
#define PJ_KEY_FALLBACK 0xffffffffu
#define PJ_KEY_LONG 0xfffffffeu      /* the strip kernel's pair mode (queries of 769 residues and more) */
#define PJ_LONG_MIN 769

/* a pair of the long class on its way into jobs: sorted by bucket key, then query length, then target length (the two halves of a job and
   the jobs of a launch finish together), then position */
typedef struct { int32_t key, len; int64_t tl, i; } plong;
static int plong_cmp(const void* a, const void* b)
{
	const plong* x = (const plong*)a; const plong* y = (const plong*)b;
	if (x->key != y->key) return x->key < y->key ? -1 : 1;
	if (x->len != y->len) return x->len < y->len ? -1 : 1;
	if (x->tl != y->tl) return x->tl < y->tl ? -1 : 1;
	return x->i < y->i ? -1 : x->i > y->i;
}
/* jobs [j0, j0 + jn) of the long class share the strip shape b; maxt: their longest target */
typedef struct { bucket b; int64_t j0, jn, maxt; } plong_bucket;
/* (scratch of one job: plong_job_bytes, above the database path, which cuts its long class by the same rule) */

static double wall_ms(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }

/* the pairs list[0 .. nl) outside the kernel's envelope: grouped by target (counting sort), their queries gathered on the device in
   chunks of at most max(budget / 8, 1 MiB) residues, one align_batch per target; CIGARs appended to the staging pool */
static int pairs_fallback(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int32_t* qidx, const int32_t* tidx,
                          const int64_t* list, int64_t nl, const ssw_gpu_params* prm, ssw_gpu_result* results, cigar_stage* st, call_acc* acc)
{
	const int32_t nt = T->count;
	int64_t* tstart = (int64_t*)calloc((size_t)nt + 1, sizeof(int64_t));
	int64_t* bytgt = (int64_t*)malloc(sizeof(int64_t) * (size_t)(nl > 0 ? nl : 1));
	ssw_gpu_result* tmp = 0; int32_t* gidx = 0; int64_t* goff = 0;
	int rc = -1;
	if (!tstart || !bytgt) { fail(c, "out of host memory%s", ""); goto out; }
	for (int64_t k = 0; k < nl; ++k) tstart[tidx[list[k]] + 1]++;
	for (int32_t t = 0; t < nt; ++t) tstart[t + 1] += tstart[t];
	{
		int64_t* pos = (int64_t*)malloc(sizeof(int64_t) * ((size_t)nt + 1));
		if (!pos) { fail(c, "out of host memory%s", ""); goto out; }
		memcpy(pos, tstart, sizeof(int64_t) * ((size_t)nt + 1));
		for (int64_t k = 0; k < nl; ++k) bytgt[pos[tidx[list[k]]]++] = list[k];      /* stable: pair order inside a target */
		free(pos);
	}
	int64_t maxgrp = 0;
	for (int32_t t = 0; t < nt; ++t) if (tstart[t + 1] - tstart[t] > maxgrp) maxgrp = tstart[t + 1] - tstart[t];
	if (maxgrp > 0x7fffffff) { fail(c, "align_pairs: %s", "more than 2^31 pairs against one target outside the fused kernel's envelope"); goto out; }
	tmp = (ssw_gpu_result*)malloc(sizeof(ssw_gpu_result) * (size_t)(maxgrp > 0 ? maxgrp : 1));
	if (!tmp) { fail(c, "out of host memory%s", ""); goto out; }
	int64_t lim = (int64_t)(c->cm_budget / 8); if (lim < ((int64_t)1 << 20)) lim = (int64_t)1 << 20;
	for (int32_t t0 = 0; t0 < nt; ) {
		/* a chunk of consecutive targets whose gathered queries stay within `lim` residues (at least one target) */
		int32_t t1 = t0; int64_t res_sum = 0;
		while (t1 < nt) {
			int64_t s = 0;
			for (int64_t k = tstart[t1]; k < tstart[t1 + 1]; ++k) s += Q->h_off[qidx[bytgt[k]] + 1] - Q->h_off[qidx[bytgt[k]]];
			if (t1 > t0 && res_sum + s > lim) break;
			res_sum += s; ++t1;
		}
		const int64_t k0 = tstart[t0], cnt = tstart[t1] - k0;
		if (cnt == 0) { t0 = t1; continue; }
		if (cnt > 0x7fffffff) { fail(c, "align_pairs: %s", "fallback chunk too large"); goto out; }
		free(gidx); free(goff);
		gidx = (int32_t*)malloc(sizeof(int32_t) * (size_t)cnt); goff = (int64_t*)malloc(sizeof(int64_t) * ((size_t)cnt + 1));
		if (!gidx || !goff) { fail(c, "out of host memory%s", ""); goto out; }
		goff[0] = 0;
		for (int64_t k = 0; k < cnt; ++k) { const int32_t q = qidx[bytgt[k0 + k]]; gidx[k] = q; goff[k + 1] = goff[k] + (Q->h_off[q + 1] - Q->h_off[q]); }
		ssw_gpu_seqs* G = seqs_new(c, goff, (int32_t)cnt);
		if (!G) goto out;
		int32_t* d_idx = (int32_t*)ssw_shim_malloc(sizeof(int32_t) * (size_t)cnt);
		ssw_seqgather_args ga; ga.src_beg = 0; ga.src = Q->d_codes; ga.src_off = Q->d_off; ga.idx = d_idx; ga.dst_off = G->d_off; ga.dst = G->d_codes; ga.count = (int32_t)cnt;
		const int ok = d_idx && !ssw_shim_h2d(d_idx, gidx, sizeof(int32_t) * (size_t)cnt, c->stream) &&
		               !ssw_shim_h2d(G->d_off, G->h_off, sizeof(int64_t) * ((size_t)cnt + 1), c->stream) &&
		               !ssw_shim_launch_seqgather(&ga, c->stream) && !ssw_shim_stream_sync(c->stream);
		ssw_shim_free(d_idx);
		if (!ok) { fail(c, "align_pairs: query gather failed: %s", ssw_shim_last_error()); ssw_gpu_seqs_free(G); goto out; }
		for (int32_t t = t0; t < t1; ++t) {
			const int64_t a0 = tstart[t] - k0, m = tstart[t + 1] - tstart[t];
			if (m == 0) continue;
			/* a view of the gathered set: this target's queries (offsets stay absolute in G's codes) */
			struct ssw_gpu_seqs V; V.ctx = c; V.d_codes = G->d_codes; V.d_off = G->d_off + a0; V.h_off = G->h_off + a0; V.count = (int32_t)m;
			V.total = V.h_off[m] - V.h_off[0];
			uint32_t* pool = 0; int64_t words = 0;
			if (align_batch_locked(c, &V, T, t, 1, prm, tmp, &pool, &words, 0)) { ssw_gpu_seqs_free(G); goto out; }      /* (the pool is always taken: offsets in pair order) */
			timing_add(acc, &c->tm);
			if (stage_append_batch(c, st, pool, words, tmp, m, bytgt + tstart[t], sizeof(int64_t), results)) { ssw_gpu_seqs_free(G); goto out; }
		}
		ssw_gpu_seqs_free(G);
		t0 = t1;
	}
	rc = 0;
out:
	free(tstart); free(bytgt); free(tmp); free(gidx); free(goff);
	return rc;
}

/* Flagged pairs inside the fused kernel's envelope: k_fillpairs gave scores and end positions (status carries SSW_OUT_WORD); the pairs that
   pass the reference's gate (src/ssw.c:900-903, 916) become a survivor list grouped by query geometry bucket (a counting sort: survivors of
   a bucket stay in record order), and the reverse pass and the traceback run over it as (query, target) jobs: survivor_phases.  rec[0 .. nrec)
   are the fill's records of the pairs pix[]; they are completed in place, CIGARs appended to the staging pool (always, like align_batch does). */
static int pairs_flagged(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int32_t* qidx, const pair_src* src,
                         const int64_t* pix, ssw_gpu_result* rec, int64_t nrec, const ssw_gpu_params* prm, const int8_t* d_mat,
                         int32_t maxmat, int32_t minmat, cigar_stage* st)
{
	win_geom geom;
	win_geom_fill(&geom, &c->kn, prm->n);
	/* bucket keys (win_bucket_key): up to SSW_RMAX + 64 + 41 for queries of the short class (<= 640 residues), SSW_RMAX + 64 + P16 / 16 for the
	   strip kernel's pair mode -- the key arrays are sized from the longest query of the list */
	int32_t maxq = 0;
	for (int64_t k = 0; k < nrec; ++k) { const int64_t i = pix[k]; const int32_t len = (int32_t)(Q->h_off[qidx[i] + 1] - Q->h_off[qidx[i]]); if (len > maxq) maxq = len; }
	const int NKEY = SSW_RMAX + 64 + (maxq + 15) / 16 + 1;
	int64_t* kfirst = (int64_t*)calloc((size_t)NKEY + 1, sizeof(int64_t));
	int64_t* kpos = (int64_t*)malloc(sizeof(int64_t) * (size_t)NKEY);
	int32_t* kp16 = (int32_t*)calloc((size_t)NKEY, sizeof(int32_t));
	int32_t* key = (int32_t*)malloc(sizeof(int32_t) * (size_t)(nrec > 0 ? nrec : 1));
	int64_t* order = (int64_t*)malloc(sizeof(int64_t) * (size_t)(nrec > 0 ? nrec : 1));
	ssw_dres* hs = 0; int32_t* hvq = 0; int64_t* poff = 0; surv_range* rg = 0;
	int rc = -1;
	if (!kfirst || !kpos || !kp16 || !key || !order) { fail(c, "out of host memory%s", ""); goto out; }
	int64_t ns = 0; int32_t maxlen = 0; int64_t maxt = 0;
	for (int64_t k = 0; k < nrec; ++k) {
		ssw_gpu_result* o = &rec[k];
		const int word = (o->status & SSW_OUT_WORD) != 0;
		o->status &= 0xffu;
		key[k] = -1;
		if (o->status != 0 || o->score1 == 0 || (prm->flag == 2 && (int)o->score1 < prm->filters)) continue;      /* ssw.c:900-903, 916 */
		const int64_t i = pix[k];
		const int32_t len = (int32_t)(Q->h_off[qidx[i] + 1] - Q->h_off[qidx[i]]);
		const int64_t tl = ps_tlen(src, T, i);
		int32_t P16q;
		const int32_t kk = win_bucket_key(&geom, len, &P16q);
		key[k] = kk | (word << 30);
		kfirst[kk + 1]++;
		if (P16q > kp16[kk]) kp16[kk] = P16q;
		if (len > maxlen) maxlen = len;
		if (tl > maxt) maxt = tl;
		++ns;
	}
	if (ns == 0) { rc = 0; goto out; }
	if (ns > 0x7fffff00) { fail(c, "%s: more than 2^31 flagged pairs in one call", src->who); goto out; }
	for (int b = 0; b < NKEY; ++b) kfirst[b + 1] += kfirst[b];
	memcpy(kpos, kfirst, sizeof(int64_t) * (size_t)NKEY);
	for (int64_t k = 0; k < nrec; ++k) if (key[k] >= 0) order[kpos[key[k] & 0xffff]++] = k;
	hs = (ssw_dres*)malloc(sizeof(ssw_dres) * (size_t)ns); hvq = (int32_t*)malloc(sizeof(int32_t) * 3 * (size_t)ns);
	if (!hs || !hvq) { fail(c, "out of host memory%s", ""); goto out; }
	for (int64_t v = 0; v < ns; ++v) {
		const int64_t k = order[v], i = pix[k];
		const ssw_gpu_result* o = &rec[k];
		ssw_dres* r = &hs[v];
		memset(r, 0, sizeof *r);
		r->score1 = o->score1; r->score2 = o->score2; r->ref_begin1 = -1; r->ref_end1 = o->ref_end1; r->read_begin1 = -1; r->read_end1 = o->read_end1;
		r->ref_end2 = o->ref_end2; r->word = (key[k] >> 30) & 1; r->want_begin = 1; r->loc_done = 1;      /* (as k_select writes them) */
		hvq[v] = qidx[i]; hvq[ns + v] = ps_tid(src, i); hvq[2 * ns + v] = (int32_t)v;      /* query, target, identity list */
	}
	ssw_dres* d_sres = (ssw_dres*)ensure(c, &c->sres, sizeof(ssw_dres) * (size_t)ns);
	int32_t* d_maps = (int32_t*)ensure(c, &c->svq, sizeof(int32_t) * 4 * (size_t)ns);      /* vq, vt, identity list, traceback job lists */
	if (!d_sres || !d_maps) goto out;
	ssw_shim_event_record(c->ev_a, c->stream);
	if (ssw_shim_h2d(d_sres, hs, sizeof(ssw_dres) * (size_t)ns, c->stream) || ssw_shim_h2d(d_maps, hvq, sizeof(int32_t) * 3 * (size_t)ns, c->stream)) {
		fail(c, "upload failed: %s", ssw_shim_last_error()); goto out;
	}
	poff = (int64_t*)malloc(sizeof(int64_t) * (size_t)ns); rg = (surv_range*)malloc(sizeof(surv_range) * (size_t)NKEY);
	if (!poff || !rg) { fail(c, "out of host memory%s", ""); goto out; }
	int nrg = 0;
	for (int kk = 0; kk < NKEY; ++kk) {
		if (kfirst[kk + 1] == kfirst[kk]) continue;
		memset(&rg[nrg], 0, sizeof rg[nrg]);
		win_bucket_shape(&rg[nrg].b, &geom, kk, kp16[kk]);
		rg[nrg].first = kfirst[kk]; rg[nrg].count = kfirst[kk + 1] - kfirst[kk];
		++nrg;
	}
	surv_in si; memset(&si, 0, sizeof si);
	si.Q = Q; si.T = T; si.prm = prm; si.d_mat = d_mat; si.maxmat = maxmat; si.minmat = minmat; si.g = &geom; si.fill_form = c->kn.fill_plain ? 0 : -1;
	si.maxlen = maxlen; si.maxt = maxt; si.d_sres = d_sres; si.d_maps = d_maps; si.ns = ns; si.d_win = src->d_win; si.rg = rg; si.nrg = nrg;
	si.check_queue = 1;
	if (survivor_phases(c, &si, hs, st, poff, &c->tm.locate_ms, &c->tm.trace_ms)) goto out;
	for (int64_t v = 0; v < ns; ++v) {      /* what the reverse pass and the traceback added to the records */
		const ssw_dres* r = &hs[v];
		ssw_gpu_result* o = &rec[order[v]];
		o->ref_begin1 = r->ref_begin1; o->read_begin1 = r->read_begin1; o->cigarLen = r->cigarLen; o->flag = (uint16_t)r->flag;
		o->edit_distance = r->nm; o->cigar_off = r->cigarLen > 0 && r->status == 0 ? poff[v] : -1;
	}
	rc = 0;
out:
	free(kfirst); free(kpos); free(kp16); free(key); free(order); free(hs); free(hvq); free(poff); free(rg);
	return rc;
}

/* (the fallbacks go back into the pair path with the temporary sets they gathered: windows_fallback -> align_pairs_locked -> pairs_core ->
   windows_fallback.  The nested call has whole targets and never gets here again.) */
static int windows_fallback(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int32_t* qidx, const pair_src* src,
                            const int64_t* list, int64_t nl, const ssw_gpu_params* prm, ssw_gpu_result* results, cigar_stage* st, call_acc* acc);

/* select mode of the pair list: the pairs are candidates in groups.  ssw_gpu_align_windows_best (k == 0): `results` has one record per
   GROUP, `sel` the selections.  ssw_gpu_align_windows_topk (k >= 1): `results` has k records per group, slot g * k + r for rank r, `pos`
   their positions in the group and `n_eligible` one count per group.  ssw_gpu_align_windows_mates (`mates`, k == 0): groups 2 f and 2 f + 1
   are the two mates of fragment f, `results` has one record per group, `mates` one selection per FRAGMENT */
typedef struct {
	const int64_t* cand_off; int64_t ngroups; int32_t min_score; ssw_gpu_best* sel;
	int32_t k, max_drop; int32_t* pos; int32_t* n_eligible;
	ssw_gpu_mates* mates; int32_t nfwd, min_insert, max_insert, unpaired_penalty, orientation;
	/* pair model (ssw_gpu_align_windows_mates_model): the caller's penalty table, n_ins = max_insert - min_insert + 1 entries; NULL: the flat rule */
	const uint16_t* ins_pen; int64_t n_ins;
	/* mate rescue (ssw_gpu_align_windows_mates_rescue; rescue_anchors == 0: none): the list is the augmented one, its four arrays are the
	   entry point's own (r_*: the same memory, writable -- pairs_core enters the non-empty rescue slots), r_slots receives the slot table */
	int32_t rescue_anchors, anchor_min_score, rescue_pad; const int32_t* mate_q;
	int32_t* r_qidx; int32_t* r_tidx; int64_t* r_tbeg; int32_t* r_tlen; ssw_gpu_rescued* r_slots;
	/* insert-size histogram (ssw_gpu_insert_hist; `ihist`): the groups, nfwd and the side table of a mates call, k_insertstat in place of
	   k_matebest, `ihist` ([3][max_span + 1]) and `icounts` the only outputs -- `results` is NULL, nothing goes on to the flagged phases */
	uint32_t* ihist; ssw_gpu_insert_counts* icounts; int32_t min_margin, max_span;
} best_mode;
/* device bytes of the per-group output behind the call-long record array: record + selection (64; mates: 48 + half of the fragment's 32) /
   k records, k positions and a count */
static size_t best_out_bytes(const best_mode* bm)
{
	if (bm->ihist) return 0;      /* (bins and counters lie behind the slot map) */
	return bm->k ? (size_t)bm->ngroups * ((sizeof(struct ssw_out_rec) + 4) * (size_t)bm->k + 4) : 64 * (size_t)bm->ngroups;
}

/* windows_fallback over the candidates list[0 .. nl) of a select-mode call, records to out[0 .. nl) in list order (the candidates' four
   arrays are compacted, so that the fallback's "pair index" is the position in the list) */
static int best_fallback(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int32_t* qidx, const pair_src* src,
                         const int64_t* list, int64_t nl, const ssw_gpu_params* prm, ssw_gpu_result* out, cigar_stage* st, call_acc* acc)
{
	int64_t* b2 = (int64_t*)malloc(sizeof(int64_t) * 2 * (size_t)nl);
	int32_t* q2 = (int32_t*)malloc(sizeof(int32_t) * 3 * (size_t)nl);
	int rc = -1;
	if (!b2 || !q2) { fail(c, "out of host memory%s", ""); goto out; }
	int64_t* id = b2 + nl; int32_t* t2 = q2 + nl; int32_t* l2 = q2 + 2 * nl;
	for (int64_t k = 0; k < nl; ++k) { const int64_t i = list[k]; q2[k] = qidx[i]; t2[k] = src->tidx[i]; b2[k] = src->tbeg[i]; l2[k] = src->tlen[i]; id[k] = k; }
	pair_src s2 = *src;
	s2.tidx = t2; s2.tbeg = b2; s2.tlen = l2; s2.d_win = 0;
	rc = windows_fallback(c, Q, T, q2, &s2, id, nl, prm, out, st, acc);
out:
	free(b2); free(q2);
	return rc;
}

/* the call-long record array of a select-mode call with room for `bytes`, its first `keep` bytes preserved (a rescue stage appends the
   records of its windows behind those the selection of anchors has read: k_copy16 moves them when the allocation has to grow) */
static unsigned char* brec_reserve(ssw_gpu_ctx* c, size_t keep, size_t bytes)
{
	dbuf* b = &c->brec;
	if (keep == 0 || !b->p || b->cap >= bytes) return (unsigned char*)ensure(c, b, bytes);
	const size_t want = bytes + bytes / 8 + 256;
	void* p = ssw_shim_malloc(want);
	if (!p) { fail(c, "device allocation failed: %s", ssw_shim_last_error()); return 0; }
	ssw_copy16_args ca; memset(&ca, 0, sizeof ca);
	ca.src = b->p; ca.dst = p; ca.n16 = (int64_t)((keep + 15) / 16);      /* (keep <= the old capacity, which ensure() rounds up by 256) */
	if (ssw_shim_launch_copy16(&ca, c->stream) || ssw_shim_stream_sync(c->stream)) {
		fail(c, "record array copy failed: %s", ssw_shim_last_error()); ssw_shim_free(p); return 0;
	}
	ssw_shim_free(b->p);
	b->p = p; b->cap = want;
	return (unsigned char*)p;
}

/* what does not change between the sublists of one call: the scores' range and which fast paths the parameters allow */
typedef struct { int32_t minmat, maxmat, bias; int kern_ok, long_ok; win_geom geom; } pair_env;

/* what the plan + fill of a sublist leaves behind for the rest of the call (pairs_core) */
typedef struct {
	int64_t* perm; int64_t nk;          /* its pairs of k_fillpairs, by (R, target-length class) */
	int64_t* fb; int64_t nfb;           /* ... outside both envelopes */
	plong* lk; int64_t nlong;           /* ... of the strip kernel's pair mode */
	int64_t* jix; int64_t nj;           /* the pair of either half of every job (-1: idle) */
	ssw_gpu_result* stage;              /* (no select mode) the fill's records, two per job */
	ssw_gpu_result* fbrec;              /* (select mode) the flag-0 records of `fb`, from the fallback */
	unsigned char* d_brec; int8_t* d_mat;
} pair_fill;
static void pair_fill_free(pair_fill* pf)
{
	free(pf->perm); free(pf->fb); free(pf->lk); free(pf->jix); free(pf->stage); free(pf->fbrec);
	memset(pf, 0, sizeof *pf);
}

/* Plan + fill of the sublist list[0 .. nl) of a pair list of np pairs (list == NULL: all of them): the classes go to key[] (the call's
   array, one entry per pair of the LIST), the jobs are launched, and in select mode the records stay on the device from record rec0 of
   the call-long array on -- two per job, then room for the fallback's, which come back in pf->fbrec --, records [0, rec0) preserved;
   `rec_extra` more records and the per-group output fit behind them.  The window table covers all np pairs: it is built here unless
   the call has one already (src->d_win). */
static int pairs_fill(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int32_t* qidx, pair_src* src, int64_t np,
                      const int64_t* list, int64_t nl, const ssw_gpu_params* prm, const pair_env* env, const best_mode* bm, uint32_t* key,
                      int64_t rec0, int64_t rec_extra, pair_fill* pf, cigar_stage* st, call_acc* acc)
{
	const int32_t minmat = env->minmat, maxmat = env->maxmat, bias = env->bias, n = prm->n;
	const int kern_ok = env->kern_ok, long_ok = env->long_ok;
	const win_geom geom = env->geom;
	/* ---- plan: counting sort of the kernel's pairs by (R, target-length class); the rest to the fallback list */
	const int64_t nkeys = (int64_t)40 * PJ_TCLS;
	int64_t* kcount = (int64_t*)calloc((size_t)nkeys + 1, sizeof(int64_t));
	int64_t* perm = (int64_t*)malloc(sizeof(int64_t) * (size_t)(nl > 0 ? nl : 1));
	int64_t* fb = 0; int64_t nfb = 0;
	plong* lk = 0; plong_bucket* lb = 0; int64_t nlong = 0; int nlb = 0;
	ssw_pjob* jobs = 0; int64_t* jix = 0; ssw_gpu_result* stage = 0;
	ssw_gpu_result* fbrec = 0;      /* select mode */
	unsigned char* d_brec = 0; int8_t* d_mat = 0; int64_t nj = 0;
	int rc = -1;
	memset(pf, 0, sizeof *pf);
	if (!kcount || !perm) { fail(c, "out of host memory%s", ""); goto done; }
	for (int64_t li = 0; li < nl; ++li) {
		const int64_t i = list ? list[li] : li;
		const int64_t ql = Q->h_off[qidx[i] + 1] - Q->h_off[qidx[i]], tl = ps_tlen(src, T, i);
		const int R = (int)((ql + 15) / 16);
		if (long_ok && ql >= PJ_LONG_MIN && ql <= PJ_LONG_MAX && tl >= 1 && tl <= 65000) {
			/* (queries of 641 .. 768 residues: neither class, the fallback) */
			int32_t P16q; bucket B;
			const int32_t kk = win_bucket_key(&geom, (int32_t)ql, &P16q);
			win_bucket_shape(&B, &geom, kk, P16q);
			if (plong_job_bytes(tl, B.strips) <= (int64_t)(c->cm_budget / 2)) { key[i] = PJ_KEY_LONG; ++nlong; continue; }
		}
		if (!kern_ok || ql < 1 || ql > 640 || tl < 1 || tl > 65000 || (int64_t)n * ((R + 3) / 4) * 256 > 65535) { key[i] = PJ_KEY_FALLBACK; ++nfb; continue; }
		key[i] = (uint32_t)((R - 1) * PJ_TCLS + (tl >> 5 < PJ_TCLS ? tl >> 5 : PJ_TCLS - 1));
		kcount[key[i] + 1]++;
	}
	for (int64_t k = 0; k < nkeys; ++k) kcount[k + 1] += kcount[k];
	const int64_t nk = kcount[nkeys];
	if (nfb > 0) { fb = (int64_t*)malloc(sizeof(int64_t) * (size_t)nfb); if (!fb) { fail(c, "out of host memory%s", ""); goto done; } }
	{
		int64_t f = 0;
		for (int64_t li = 0; li < nl; ++li) {
			const int64_t i = list ? list[li] : li;
			if (key[i] == PJ_KEY_FALLBACK) fb[f++] = i;
			else if (key[i] != PJ_KEY_LONG) perm[kcount[key[i]]++] = i;      /* kcount[k] ends as the end of class k */
		}
	}
	if (nlong > 0) {
		lk = (plong*)malloc(sizeof(plong) * (size_t)nlong); lb = (plong_bucket*)malloc(sizeof(plong_bucket) * (size_t)nlong);
		if (!lk || !lb) { fail(c, "out of host memory%s", ""); goto done; }
		int64_t f = 0;
		for (int64_t li = 0; li < nl; ++li) {
			const int64_t i = list ? list[li] : li;
			if (key[i] != PJ_KEY_LONG) continue;
			int32_t P16q;
			lk[f].len = (int32_t)(Q->h_off[qidx[i] + 1] - Q->h_off[qidx[i]]); lk[f].key = win_bucket_key(&geom, lk[f].len, &P16q);
			lk[f].tl = ps_tlen(src, T, i); lk[f].i = i; ++f;
		}
		qsort(lk, (size_t)nlong, sizeof(plong), plong_cmp);
	}

	if (bm && nfb > 0) {      /* select mode: what the candidates outside the envelope score, before the device holds anything of this call */
		ssw_gpu_params p0 = *prm; p0.flag = 0;
		fbrec = (ssw_gpu_result*)malloc(sizeof(ssw_gpu_result) * (size_t)nfb);
		if (!fbrec) { fail(c, "out of host memory%s", ""); goto done; }
		if (best_fallback(c, Q, T, qidx, src, fb, nfb, &p0, fbrec, st, acc)) goto done;
		memset(&c->tm, 0, sizeof c->tm);
	}
	if (nk + nlong > 0) {
		/* jobs: neighbours of one R (sorted by target length: the two halves and the chains of a workgroup finish together) */
		const int64_t njmax = nk / 2 + 40 + nlong;
		jobs = (ssw_pjob*)malloc(sizeof(ssw_pjob) * (size_t)njmax);
		jix = (int64_t*)malloc(sizeof(int64_t) * 2 * (size_t)njmax);
		if (!jobs || !jix) { fail(c, "out of host memory%s", ""); goto done; }
		int64_t rfirst[41], maxt[40];
		for (int R = 1; R <= 40; ++R) {
			const int64_t lo = R == 1 ? 0 : kcount[(int64_t)(R - 1) * PJ_TCLS - 1], hi = kcount[(int64_t)R * PJ_TCLS - 1];
			rfirst[R - 1] = nj; maxt[R - 1] = 0;
			for (int64_t k = lo; k < hi; k += 2) {
				const int64_t pa = perm[k], pb = k + 1 < hi ? perm[k + 1] : -1;
				ssw_pjob* j = &jobs[nj];
				j->qa = qidx[pa]; j->ta = ps_tid(src, pa);
				j->qb = pb >= 0 ? qidx[pb] : -1; j->tb = ps_tid(src, pb >= 0 ? pb : pa);
				jix[2 * nj] = pa; jix[2 * nj + 1] = pb;
				const int64_t L = ps_tlen(src, T, pa), Lb = pb >= 0 ? ps_tlen(src, T, pb) : 0;
				if (L > maxt[R - 1]) maxt[R - 1] = L;
				if (Lb > maxt[R - 1]) maxt[R - 1] = Lb;
				++nj;
			}
		}
		rfirst[40] = nj;
		/* ... then the long class in the same numbering: neighbours of one bucket (win_bucket_key: jobs of several strips pair queries of ONE
		   padded length; a query without a partner runs with an idle high half) */
		for (int64_t k = 0; k < nlong; ) {
			int64_t k1 = k; int32_t p16 = 0;
			plong_bucket* L = &lb[nlb++];
			memset(L, 0, sizeof *L);
			L->j0 = nj;
			while (k1 < nlong && lk[k1].key == lk[k].key) { const int32_t P = (lk[k1].len + 15) / 16 * 16; if (P > p16) p16 = P; if (lk[k1].tl > L->maxt) L->maxt = lk[k1].tl; ++k1; }
			win_bucket_shape(&L->b, &geom, lk[k].key, p16);
			for (; k < k1; k += 2) {
				const int64_t pa = lk[k].i, pb = k + 1 < k1 ? lk[k + 1].i : -1;
				ssw_pjob* j = &jobs[nj];
				j->qa = qidx[pa]; j->ta = ps_tid(src, pa);
				j->qb = pb >= 0 ? qidx[pb] : -1; j->tb = ps_tid(src, pb >= 0 ? pb : pa);
				jix[2 * nj] = pa; jix[2 * nj + 1] = pb;
				++nj;
			}
			k = k1;
			L->jn = nj - L->j0;
		}
		/* the call's small inputs: matrix + jobs in one upload */
		const size_t hdr_mat = ((size_t)n * n + 15) / 16 * 16;
		unsigned char* d_hdr = (unsigned char*)ensure(c, &c->pairs, hdr_mat + sizeof(ssw_pjob) * (size_t)nj);
		int32_t* d_cnt = (int32_t*)ensure(c, &c->need, DB_COUNTERS * sizeof(int32_t));
		if (!bm) stage = (ssw_gpu_result*)malloc(sizeof(ssw_gpu_result) * 2 * (size_t)nj);
		if (!d_hdr || !d_cnt) goto done;
		if (!bm && !stage) { fail(c, "out of host memory%s", ""); goto done; }
		/* select mode: the records of ALL fill launches stay on the device (two per job, then the fallback's), followed by the per-group output.
		   An input / output of the call like the window table, not scratch under the budget: 48 bytes per candidate; 64 per group, or with
		   k ranks (ssw_gpu_align_windows_topk) 52 k + 4 per group */
		if (bm && !(d_brec = brec_reserve(c, sizeof(struct ssw_out_rec) * (size_t)rec0,
		                                  sizeof(struct ssw_out_rec) * (size_t)(rec0 + 2 * nj + nfb + rec_extra) + best_out_bytes(bm)))) goto done;
		d_mat = (int8_t*)d_hdr;
		ssw_pjob* d_jobs = (ssw_pjob*)(d_hdr + hdr_mat);
		c->nev = 0;
		ssw_shim_event_record(c->ev_t0, c->stream);
		if (ssw_shim_h2d(d_mat, prm->mat, (size_t)n * n, c->stream) || ssw_shim_h2d(d_jobs, jobs, sizeof(ssw_pjob) * (size_t)nj, c->stream) ||
		    ssw_shim_memset(d_cnt, 0, DB_COUNTERS * sizeof(int32_t), c->stream)) { fail(c, "upload failed: %s", ssw_shim_last_error()); goto done; }
		if (src->tbeg && !src->d_win) {
			/* the window table: the caller's three arrays go up as they are (16 bytes per pair), k_wintab adds the resident offsets */
			unsigned char* d_w = (unsigned char*)ensure(c, &c->wtab, 32 * (size_t)np);
			if (!d_w) goto done;
			ssw_wintab_args wa; memset(&wa, 0, sizeof wa);
			wa.win = (ssw_win*)d_w; wa.tbeg = (const int64_t*)(d_w + 16 * (size_t)np); wa.tidx = (const int32_t*)(d_w + 24 * (size_t)np);
			wa.tlen = (const int32_t*)(d_w + 28 * (size_t)np); wa.toff = T->d_off; wa.count = np;
			if (ssw_shim_h2d((void*)wa.tbeg, src->tbeg, 8 * (size_t)np, c->stream) || ssw_shim_h2d((void*)wa.tidx, src->tidx, 4 * (size_t)np, c->stream) ||
			    ssw_shim_h2d((void*)wa.tlen, src->tlen, 4 * (size_t)np, c->stream) || ssw_shim_launch_wintab(&wa, c->stream)) {
				fail(c, "window table failed: %s", ssw_shim_last_error()); goto done;
			}
			src->d_win = wa.win;
		}
		const uint32_t gapO2 = (uint32_t)prm->gapO * 0x10001u, gapE2 = (uint32_t)prm->gapE * 0x10001u;
		int64_t kcells = 0, kbest = 0;
		for (int R = 1; R <= 40; ++R) {
			const int64_t j0 = rfirst[R - 1], jn = rfirst[R] - j0;
			if (jn == 0) continue;
			const int nch = ssw_shim_fillpairs_nch(R, n);
			if (nch < 1) { fail(c, "%s: no k_fillpairs geometry for this alphabet", src->who); goto done; }
			const int64_t stride = (maxt[R - 1] + 15) / 16 * 16 + 16;
			/* scratch of a job: its two column-maximum rows + two records; jobs per launch: what half the budget holds, whole workgroups */
			const int64_t per_job = 8 * stride + 2 * (int64_t)sizeof(ssw_gpu_result);
			int64_t jpl = (int64_t)(c->cm_budget / 2) / per_job;
			const int nch_l = jpl < nch ? (jpl > 1 ? (int)jpl : 1) : nch;      /* a small budget: fewer chains per workgroup (one job at the least) */
			jpl = jpl / nch_l * nch_l;
			if (jpl < nch_l) jpl = nch_l;
			if (jpl > jn) jpl = jn;
			uint32_t* d_cm16 = (uint32_t*)ensure(c, &c->cm16, (size_t)(4 * stride * jpl));
			uint32_t* d_cm8 = (uint32_t*)ensure(c, &c->cm8, (size_t)(4 * stride * jpl));
			struct ssw_out_rec* d_out = bm ? (struct ssw_out_rec*)d_brec + rec0 : (struct ssw_out_rec*)ensure(c, &c->res, sizeof(struct ssw_out_rec) * 2 * (size_t)jpl);
			if (!d_cm16 || !d_cm8 || !d_out) goto done;
			int32_t fr_base = 0, fr_kmask = 0;
			const int fr = !c->kn.db_plain && ssw_frame_params(&c->kn, (int64_t)16 * R * maxmat, prm->gapO, prm->gapE, minmat, 16, &fr_base, &fr_kmask);
			int64_t rcells = 0;
			for (int64_t a0 = 0; a0 < jn; a0 += jpl) {
				ssw_fillpairs_args fa; memset(&fa, 0, sizeof fa);
				fa.qcodes = Q->d_codes; fa.qoff = Q->d_off; fa.tcodes = T->d_codes; fa.toff = T->d_off; fa.win = src->d_win; fa.jobs = d_jobs + j0 + a0;
				fa.njobs = jn - a0 < jpl ? jn - a0 : jpl; fa.mat = d_mat; fa.n = n; fa.gapO2 = gapO2; fa.gapE2 = gapE2;
				fa.cm16 = d_cm16; fa.cm8 = d_cm8; fa.cm_stride = stride; fa.maskLen = prm->maskLen; fa.bias = bias; fa.score_size = prm->score_size;
				fa.out = bm ? d_out + 2 * (j0 + a0) : d_out; fa.counters = d_cnt; fa.form = fr; fa.fr_base = fr_base; fa.fr_kmask = fr_kmask;
				fa.nch = nch_l; fa.mark_word = prm->flag != 0;
				void* e0 = next_event(c); void* e1 = next_event(c);
				ssw_shim_event_record(e0, c->stream);
				if (ssw_shim_launch_fillpairs(R, &fa, c->stream)) { fail(c, "fillpairs launch failed: %s", ssw_shim_last_error()); goto done; }
				ssw_shim_event_record(e1, c->stream);
				/* same stream: the next launch of the loop reuses d_out / d_cm* only after this download */
				if (!bm && ssw_shim_d2h(stage + 2 * (j0 + a0), d_out, sizeof(struct ssw_out_rec) * 2 * (size_t)fa.njobs, c->stream)) { fail(c, "result download failed: %s", ssw_shim_last_error()); goto done; }
				c->tm.fill_launches++;
				for (int64_t j = j0 + a0; j < j0 + a0 + fa.njobs; ++j) {
					const int64_t La = ps_tlen(src, T, jix[2 * j]), Lb = jix[2 * j + 1] >= 0 ? ps_tlen(src, T, jix[2 * j + 1]) : 0;
					rcells += (int64_t)16 * R * 2 * (La > Lb ? La : Lb);
				}
			}
			kcells += rcells;
			char nm[48];
			snprintf(nm, sizeof nm, "k_fillpairs<%d,%s>", R, fr ? "frame" : "int16+max3");
			note_fill_kernel(c, rcells, &kbest, nm, fr ? 7.5 : 9.5, R, 1);
		}
		/* ---- the long class: per bucket, launches of the strip kernel's pair mode behind its work queue, each followed by k_reduce_pairs
		   (records as k_fillpairs leaves them, two per job, into the same arrays) */
		for (int b = 0; b < nlb; ++b) {
			const plong_bucket* L = &lb[b]; const bucket* B = &L->b;
			const int64_t stride = plong_cm_stride(L->maxt), bcols = plong_bnd_cols(L->maxt);
			int64_t jpl = (int64_t)(c->cm_budget / 2) / plong_job_bytes(L->maxt, B->strips);      /* (>= 1: every pair passed the planner's gate with its own target) */
			if (jpl < 1) jpl = 1;
			if (jpl > L->jn) jpl = L->jn;
			if (jpl * B->strips > 0x7ffffff0 / 2) jpl = 0x7ffffff0 / 2 / B->strips;
			uint32_t* d_cm16 = (uint32_t*)ensure(c, &c->cm16, (size_t)(4 * stride * jpl));
			uint32_t* d_cm8 = (uint32_t*)ensure(c, &c->cm8, (size_t)(4 * stride * jpl));
			uint32_t* d_bnd = (uint32_t*)ensure(c, &c->bnd, (size_t)(16 * bcols * jpl));
			int32_t* d_cand = (int32_t*)ensure(c, &c->cand, (size_t)(32 * jpl));
			struct ssw_out_rec* d_out = bm ? (struct ssw_out_rec*)d_brec + rec0 : (struct ssw_out_rec*)ensure(c, &c->res, sizeof(struct ssw_out_rec) * 2 * (size_t)jpl);
			if (!d_cm16 || !d_cm8 || !d_bnd || !d_cand || !d_out) goto done;
			int32_t fr_base = 0, fr_kmask = 0;
			const int xform = !c->kn.fill_plain && ssw_frame_params(&c->kn, (int64_t)B->P16 * (maxmat > 0 ? maxmat : 0), prm->gapO, prm->gapE, minmat, 64, &fr_base, &fr_kmask) ? 3 : 0;
			/* wavefronts of the launch: the occupancy of the WINDOW pass of this R, which has the pair mode's LDS footprint (two target rings) but
			   fewer registers -- where registers bound the pair mode (R = 4, frame form: 3 per SIMD against 4) some wavefronts of the grid start
			   when others end.  Harmless: tickets are drawn in dependency order, a waiting strip's predecessor was drawn by a wavefront that runs. */
			const int qgrid = chainq_grid(c, B->R, 1, n);
			const int64_t rows = (int64_t)64 * (B->tailR ? B->R * (B->strips - 1) + B->tailR : B->R * B->strips);
			int64_t bcells = 0;
			for (int64_t a0 = 0; a0 < L->jn; a0 += jpl) {
				const int64_t nl = L->jn - a0 < jpl ? L->jn - a0 : jpl;
				ssw_chainx_args xa; memset(&xa, 0, sizeof xa);
				xa.qcodes = Q->d_codes; xa.qoff = Q->d_off; xa.mat = d_mat; xa.n = n; xa.gapO2 = gapO2; xa.gapE2 = gapE2; xa.gapE = prm->gapE; xa.maxmat = maxmat;
				xa.njobs = (int32_t)nl; xa.pjobs = d_jobs + L->j0 + a0; xa.vm.tcodes = T->d_codes; xa.vm.toff = T->d_off; xa.vm.win = src->d_win;
				xa.ntiles = 1; xa.cm16 = d_cm16; xa.cm8 = d_cm8; xa.cm_stride = stride; xa.bnd = d_bnd; xa.bnd_stride = bcols; xa.cand = d_cand; xa.lanes = 64;
				if (chainq_prepare(c, &xa, B->strips, nl, qgrid)) goto done;
				xa.form = xform; xa.fr_base = fr_base; xa.fr_kmask = fr_kmask; xa.tail_R = B->tailR;
				if (c->kn.debug) fprintf(stderr, "[ssw_gpu] chainq pair fill: R %d (last strip %d), %lld jobs x %d strips, %d wavefronts, %s tickets, form %d\n",
				                                     B->R, B->tailR ? B->tailR : B->R, (long long)nl, B->strips, qgrid, xa.whole_jobs ? "job" : "strip", xa.form);
				void* e0 = next_event(c); void* e1 = next_event(c);
				ssw_shim_event_record(e0, c->stream);
				if (ssw_shim_launch_chainq(B->R, 2, &xa, qgrid, c->stream)) { fail(c, "fill launch failed: %s", ssw_shim_last_error()); goto done; }
				ssw_shim_event_record(e1, c->stream);
				ssw_reduce_pairs_args ra; memset(&ra, 0, sizeof ra);
				ra.jobs = xa.pjobs; ra.njobs = xa.njobs; ra.qoff = Q->d_off; ra.toff = T->d_off; ra.win = src->d_win; ra.cm16 = d_cm16; ra.cm8 = d_cm8; ra.cm_stride = stride;
				ra.cand = d_cand; ra.maskLen = prm->maskLen; ra.bias = bias; ra.score_size = prm->score_size;
				ra.out = bm ? d_out + 2 * (L->j0 + a0) : d_out; ra.counters = d_cnt; ra.mark_word = prm->flag != 0; ra.err = xa.err;
				if (ssw_shim_launch_reduce_pairs(&ra, c->stream)) { fail(c, "reduce launch failed: %s", ssw_shim_last_error()); goto done; }
				/* same stream: the next launch of the loop reuses the scratch only after this download */
				if (!bm && ssw_shim_d2h(stage + 2 * (L->j0 + a0), d_out, sizeof(struct ssw_out_rec) * 2 * (size_t)nl, c->stream)) { fail(c, "result download failed: %s", ssw_shim_last_error()); goto done; }
				c->tm.fill_launches++;
				for (int64_t j = L->j0 + a0; j < L->j0 + a0 + nl; ++j) {
					const int64_t La = ps_tlen(src, T, jix[2 * j]), Lb = jix[2 * j + 1] >= 0 ? ps_tlen(src, T, jix[2 * j + 1]) : 0;
					bcells += rows * 2 * (La > Lb ? La : Lb);
				}
			}
			kcells += bcells;
			char nm[48];      /* (R <= 16, strips <= 256, tail <= 4: at most 46 characters; snprintf cuts anything longer) */
			const int nlen = B->tailR ? snprintf(nm, sizeof nm, "k_chainq<%d,pairs,%s> x %d strips + 1 of %d", B->R, xform == 3 ? "frame" : "int16", B->strips - 1, B->tailR)
			                          : snprintf(nm, sizeof nm, "k_chainq<%d,pairs,%s> x %d strips", B->R, xform == 3 ? "frame" : "int16", B->strips);
			if (nlen >= (int)sizeof nm && c->kn.debug) fprintf(stderr, "[ssw_gpu] fill kernel name cut to %d characters\n", (int)sizeof nm - 1);
			note_fill_kernel(c, bcells, &kbest, nm, xform == 3 ? 6.5 : 9.0, B->R, B->strips);
		}
		int32_t cnt[DB_COUNTERS] = { 0, 0, 0, 0 };
		ssw_shim_event_record(c->ev_d, c->stream);
		if (ssw_shim_d2h(cnt, d_cnt, sizeof cnt, c->stream) || ssw_shim_stream_sync(c->stream)) { fail(c, "result download failed: %s", ssw_shim_last_error()); goto done; }
		if (chainq_check(c)) goto done;      /* (the long class: a strip that gave up waiting, or a best cell that is not the maximum's first column) */
		for (int e = 0; e + 1 < c->nev; e += 2) c->tm.fill_ms += ssw_shim_event_elapsed_ms(c->ev[e], c->ev[e + 1]);
		c->tm.fill_cells = kcells; c->tm.n_word = cnt[0]; c->tm.n_byte = cnt[1];      /* (the reduction is fused into the fill: reduce_ms stays 0) */
	}
	/* (select mode: a sublist without a fill launch still has its place in the record array) */
	if (bm && !d_brec && !(d_brec = brec_reserve(c, sizeof(struct ssw_out_rec) * (size_t)rec0,
	                                             sizeof(struct ssw_out_rec) * (size_t)(rec0 + nfb + rec_extra) + best_out_bytes(bm)))) goto done;
	for (int64_t k = 0; k < nk; ++k) {      /* (the fallback's cells came with its batches) */
		const int64_t i = perm[k]; acc->t.cells += (Q->h_off[qidx[i] + 1] - Q->h_off[qidx[i]]) * ps_tlen(src, T, i); }
	for (int64_t k = 0; k < nlong; ++k) acc->t.cells += (int64_t)lk[k].len * lk[k].tl;
	pf->perm = perm; pf->nk = nk; pf->fb = fb; pf->nfb = nfb; pf->lk = lk; pf->nlong = nlong; pf->jix = jix; pf->nj = nj;
	pf->stage = stage; pf->fbrec = fbrec; pf->d_brec = d_brec; pf->d_mat = d_mat;
	perm = 0; fb = 0; lk = 0; jix = 0; stage = 0; fbrec = 0;
	rc = 0;
done:
	free(kcount); free(perm); free(fb); free(lk); free(lb); free(jobs); free(jix); free(stage); free(fbrec);
	return rc;
}

/* The pair list of the entry points, arguments checked by the caller: planning and launch loop (pairs_fill), flagged phases, fallback and
   pool assembly.
   They differ only in where a pair's target starts and how long it is (pair_src) -- and, with `bm` (select mode), in what happens to the
   fill's records: they stay on the device in one call-long array, k_groupbest (k_grouptopk: the best k) selects per group after the last
   fill launch, one record and one selection per group (k records and positions) come to the host, and only the winners go on to the
   flagged phases.  The candidates outside the envelope take
   the fallback at flag 0 FIRST (their records join the device array, so that the selection happens in one place) and, where they win and
   flag != 0, once more with the caller's flag.
   Mate rescue (bm->rescue_anchors = A > 0): the list is the AUGMENTED one -- the last A candidates of every group are rescue slots, empty
   (tlen 0) on entry.  The first plan + fill covers the caller's candidates; k_materescue writes the slots; the non-empty ones are entered
   into the list (the caller of pairs_core owns the four arrays) and take a second plan + fill, their records appended to the device
   array; the empty ones share one all-zero record (score 0: never eligible); k_matebest and the flagged tail then see one list. */
static int pairs_core(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int32_t* qidx, pair_src* src,
                      int64_t np, const ssw_gpu_params* prm, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words,
                      const best_mode* bm)
{
	const int32_t* const tidx = src->tidx;
	if (cigar_pool) *cigar_pool = 0;
	if (cigar_words) *cigar_words = 0;
	memset(&c->tm, 0, sizeof c->tm);
	if (np == 0) return 0;
	const double t_start = wall_ms();
	ssw_shim_set_device(c->device);
	knobs_load(&c->kn);

	pair_env env; memset(&env, 0, sizeof env);
	mat_range(prm, &env.minmat, &env.maxmat, &env.bias);
	const int32_t n = prm->n, minmat = env.minmat, maxmat = env.maxmat;
	/* (flagged pairs: the window kernels reach a job's target through a 64-bit base and keep their column indices relative to it, so the size
	   of the resident set does not matter -- unlike the flagged database search's survivors) */
	env.kern_ok = prm->gapO > prm->gapE && n <= SSW_MAX_N && maxmat <= 49 && !c->kn.no_db;
	/* the strip kernel's pair mode (k_chainq<R,pairs,..>): no max(mat) gate -- ssw_frame_params picks the form per bucket */
	win_geom_fill(&env.geom, &c->kn, n);
	env.long_ok = prm->gapO > prm->gapE && n <= SSW_MAX_N && !c->kn.no_db && env.geom.xlanes == 64 && env.geom.xrmax <= 16;

	uint32_t* key = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)np);
	pair_fill pf, pf2; memset(&pf, 0, sizeof pf); memset(&pf2, 0, sizeof pf2);
	int32_t* slot = 0; int64_t* wlist = 0; ssw_gpu_result* wrec = 0; int64_t* rlist = 0;      /* select mode */
	unsigned char* d_brec = 0; int8_t* d_mat = 0;
	const int64_t nout = bm ? bm->ngroups * (bm->k ? bm->k : 1) : np;
	const int32_t RA = bm ? bm->rescue_anchors : 0;
	cigar_stage st; memset(&st, 0, sizeof st);
	call_acc acc; memset(&acc, 0, sizeof acc);
	int64_t nresc = 0; double rescue_ms = 0;
	int rc = -1;
	if (!key) { fail(c, "out of host memory%s", ""); goto done; }
	int64_t nl1 = np;
	if (RA) {      /* the caller's candidates; a rescue slot that stays empty never wins, its class does not matter */
		rlist = (int64_t*)malloc(sizeof(int64_t) * (size_t)np);
		if (!rlist) { fail(c, "out of host memory%s", ""); goto done; }
		nl1 = 0;
		for (int64_t g = 0; g < bm->ngroups; ++g) {
			const int64_t e = bm->cand_off[g + 1] - RA;
			for (int64_t i = bm->cand_off[g]; i < e; ++i) rlist[nl1++] = i;
			for (int64_t i = e; i < e + RA; ++i) key[i] = PJ_KEY_FALLBACK;
		}
	}
	if (pairs_fill(c, Q, T, qidx, src, np, RA ? rlist : 0, nl1, prm, &env, bm, key, 0, RA ? 1 : 0, &pf, &st, &acc)) goto done;
	d_brec = pf.d_brec; d_mat = pf.d_mat;
	const int64_t nj = pf.nj, nfb = pf.nfb;
	int64_t* const jix = pf.jix; int64_t* const fb = pf.fb; ssw_gpu_result* const stage = pf.stage;
	if (!bm && nj > 0) {
		/* the records of the pairs in job order (stage holds two per job; an idle high half is dropped) */
		int64_t nrec = 0;
		for (int64_t j = 0; j < nj; ++j)
			for (int h = 0; h < 2; ++h) if (jix[2 * j + h] >= 0) { stage[nrec] = stage[2 * j + h]; jix[nrec] = jix[2 * j + h]; ++nrec; }
		if (prm->flag != 0 && pairs_flagged(c, Q, T, qidx, src, jix, stage, nrec, prm, d_mat, maxmat, minmat, &st)) goto done;
		for (int64_t k = 0; k < nrec; ++k) results[jix[k]] = stage[k];
		timing_add(&acc, &c->tm);
	}
	if (bm) {
		/* ---- select: candidate -> record slot, k_groupbest (k_grouptopk, k_matebest), one selection + one record (k positions + k records) per group to the host */
		const int64_t ng = bm->ngroups;
		int64_t nrecs = 2 * nj + nfb + (RA ? 1 : 0);      /* records of the call on the device (rescue: the last one is the empty slots') */
		/* (4 bytes per candidate, 8 per group; mates: 16 more per candidate for the side table -- tbeg, tidx, length | strand --, and behind it
		   the pair model's penalty table, 2 bytes per entry) */
		const int side = bm->mates || bm->ihist;      /* the calls with a side table */
		const size_t map_bytes = 8 * ((size_t)ng + 1) + (side ? 20 : 4) * (size_t)np;
		/* (insert histogram: 3 * (max_span + 1) bins and SSW_ISTAT_COUNTERS counters, 32-bit, where a pair model's table would lie) */
		const size_t istat_bytes = bm->ihist ? 4 * (3 * ((size_t)bm->max_span + 1) + SSW_ISTAT_COUNTERS) : 0;
		unsigned char* d_map = (unsigned char*)ensure(c, &c->bmap, map_bytes + (bm->ins_pen ? 2 * (size_t)bm->n_ins : 0) + istat_bytes);
		slot = (int32_t*)malloc(sizeof(int32_t) * (side ? 2 : 1) * (size_t)np);
		if (!d_map) goto done;
		if (!slot) { fail(c, "out of host memory%s", ""); goto done; }
		if (RA) for (int64_t g = 0; g < ng; ++g) for (int64_t i = bm->cand_off[g + 1] - RA; i < bm->cand_off[g + 1]; ++i) slot[i] = (int32_t)(nrecs - 1);
		for (int64_t j = 0; j < nj; ++j)
			for (int h = 0; h < 2; ++h) if (jix[2 * j + h] >= 0) slot[jix[2 * j + h]] = (int32_t)(2 * j + h);
		for (int64_t f = 0; f < nfb; ++f) slot[fb[f]] = (int32_t)(2 * nj + f);
		const int32_t K = bm->k;
		const struct ssw_out_rec* d_rec = (const struct ssw_out_rec*)d_brec;
		const int64_t* d_off = (const int64_t*)d_map; const int64_t* d_tbeg = (const int64_t*)(d_map + 8 * ((size_t)ng + 1));      /* (mates only) */
		const int32_t* d_slot = (const int32_t*)(d_map + 8 * ((size_t)ng + 1) + (side ? 8 * (size_t)np : 0));
		ssw_gpu_result* const fbrec = pf.fbrec;
		if ((nfb > 0 && ssw_shim_h2d((void*)(d_rec + 2 * nj), fbrec, sizeof(ssw_gpu_result) * (size_t)nfb, c->stream)) ||
		    ssw_shim_h2d((void*)d_off, bm->cand_off, 8 * ((size_t)ng + 1), c->stream) || ssw_shim_h2d((void*)d_slot, slot, 4 * (size_t)np, c->stream)) {
			fail(c, "upload failed: %s", ssw_shim_last_error()); goto done;
		}
		if (side) {      /* the side table behind the slot map: [np] targets, [np] query length | minus strand << 31 */
			uint32_t* ls = (uint32_t*)slot + np;
			for (int64_t i = 0; i < np; ++i) ls[i] = (uint32_t)(Q->h_off[qidx[i] + 1] - Q->h_off[qidx[i]]) | (qidx[i] >= bm->nfwd ? 0x80000000u : 0u);
			if (ssw_shim_h2d((void*)d_tbeg, src->tbeg, 8 * (size_t)np, c->stream) || ssw_shim_h2d((void*)(d_slot + np), tidx, 4 * (size_t)np, c->stream) ||
			    ssw_shim_h2d((void*)(d_slot + 2 * np), ls, 4 * (size_t)np, c->stream)) { fail(c, "upload failed: %s", ssw_shim_last_error()); goto done; }
			/* (once per call, before the rescue stage: k_materescue does not read it, k_matebest does, on the same stream) */
			if (bm->ins_pen && ssw_shim_h2d(d_map + map_bytes, bm->ins_pen, 2 * (size_t)bm->n_ins, c->stream)) {
				fail(c, "upload failed: %s", ssw_shim_last_error()); goto done;
			}
		}
		if (RA) {
			/* ---- rescue: k_materescue over the caller's candidates, the slot table (24 bytes per slot) to the host, the non-empty slots
			   through a plan + fill of their own behind the records the device holds */
			unsigned char* d_rs = (unsigned char*)ensure(c, &c->res, sizeof(ssw_gpu_rescued) * (size_t)ng * RA + 4 * (size_t)ng);
			if (!d_rs) goto done;
			ssw_materescue_args ra; memset(&ra, 0, sizeof ra);
			ra.m.rec = d_rec; ra.m.cand_off = d_off; ra.m.slot = d_slot; ra.m.tbeg = d_tbeg; ra.m.tidx = d_slot + np; ra.m.len_strand = (const uint32_t*)(d_slot + 2 * np);
			ra.m.nfrag = ng / 2; ra.m.min_score = bm->min_score; ra.m.min_insert = bm->min_insert; ra.m.max_insert = bm->max_insert;
			ra.m.unpaired_penalty = bm->unpaired_penalty; ra.m.orientation = bm->orientation;
			ra.slots = (struct ssw_rescue_slot*)d_rs; ra.mate_q = (const int32_t*)(d_rs + sizeof(ssw_gpu_rescued) * (size_t)ng * RA);
			ra.qoff = Q->d_off; ra.toff = T->d_off; ra.nfwd = bm->nfwd; ra.max_anchors = RA; ra.anchor_min_score = bm->anchor_min_score;
			ra.rescue_pad = bm->rescue_pad; ra.side_tbeg = (int64_t*)d_tbeg; ra.side_tidx = (int32_t*)(d_slot + np); ra.side_ls = (uint32_t*)(d_slot + 2 * np);
			ra.win = (ssw_win*)src->d_win;
			void* e0 = next_event(c); void* e1 = next_event(c);
			if (ssw_shim_memset((void*)(d_rec + (nrecs - 1)), 0, sizeof(struct ssw_out_rec), c->stream) ||
			    ssw_shim_h2d((void*)ra.mate_q, bm->mate_q, 4 * (size_t)ng, c->stream)) { fail(c, "upload failed: %s", ssw_shim_last_error()); goto done; }
			ssw_shim_event_record(e0, c->stream);
			if (ssw_shim_launch_materescue(&ra, c->stream)) { fail(c, "materescue launch failed: %s", ssw_shim_last_error()); goto done; }
			ssw_shim_event_record(e1, c->stream);
			if (ssw_shim_d2h(bm->r_slots, ra.slots, sizeof(ssw_gpu_rescued) * (size_t)ng * RA, c->stream) || ssw_shim_stream_sync(c->stream)) {
				fail(c, "result download failed: %s", ssw_shim_last_error()); goto done;
			}
			rescue_ms = ssw_shim_event_elapsed_ms(e0, e1);
			for (int64_t g = 0; g < ng; ++g)
				for (int32_t r = 0; r < RA; ++r) {
					const ssw_gpu_rescued* s = &bm->r_slots[g * RA + r];
					if (s->tlen <= 0) continue;
					const int64_t i = bm->cand_off[g + 1] - RA + r;
					bm->r_qidx[i] = s->qidx; bm->r_tidx[i] = s->tidx; bm->r_tbeg[i] = s->tbeg; bm->r_tlen[i] = s->tlen;
					rlist[nresc++] = i;
				}
			if (nresc > 0) {
				timing_add(&acc, &c->tm);
				memset(&c->tm, 0, sizeof c->tm);
				const int64_t rec0 = nrecs;
				if (pairs_fill(c, Q, T, qidx, src, np, rlist, nresc, prm, &env, bm, key, rec0, 0, &pf2, &st, &acc)) goto done;
				d_brec = pf2.d_brec; d_rec = (const struct ssw_out_rec*)d_brec;
				if (pf2.d_mat) d_mat = pf2.d_mat;
				else if (d_mat) {      /* (the fallback's nested calls used the workspace the matrix of the first fill lay in) */
					if (!(d_mat = (int8_t*)ensure(c, &c->pairs, ((size_t)n * n + 15) / 16 * 16))) goto done;
					if (ssw_shim_h2d(d_mat, prm->mat, (size_t)n * n, c->stream)) { fail(c, "upload failed: %s", ssw_shim_last_error()); goto done; }
				}
				for (int64_t j = 0; j < pf2.nj; ++j)
					for (int h = 0; h < 2; ++h) if (pf2.jix[2 * j + h] >= 0) slot[pf2.jix[2 * j + h]] = (int32_t)(rec0 + 2 * j + h);
				for (int64_t f = 0; f < pf2.nfb; ++f) slot[pf2.fb[f]] = (int32_t)(rec0 + 2 * pf2.nj + f);
				nrecs = rec0 + 2 * pf2.nj + pf2.nfb;
				if ((pf2.nfb > 0 && ssw_shim_h2d((void*)(d_rec + rec0 + 2 * pf2.nj), pf2.fbrec, sizeof(ssw_gpu_result) * (size_t)pf2.nfb, c->stream)) ||
				    ssw_shim_h2d((void*)d_slot, slot, 4 * (size_t)np, c->stream)) { fail(c, "upload failed: %s", ssw_shim_last_error()); goto done; }
			}
		}
		unsigned char* d_sel = d_brec + sizeof(struct ssw_out_rec) * (size_t)nrecs;      /* best: [ng] records, [ng] selections; top-k: [nout] records, [nout] positions, [ng] counts */
		if (bm->ihist) {
			/* ---- insert histogram: bins and counters zeroed on the call's stream, k_insertstat over a bounded grid (four workgroups per
			   compute unit: every row strides over the fragments and the workgroup issues one atomic per counter), one download */
			ssw_insertstat_args ia; memset(&ia, 0, sizeof ia);
			ia.m.rec = d_rec; ia.m.cand_off = d_off; ia.m.slot = d_slot; ia.m.tbeg = d_tbeg; ia.m.tidx = d_slot + np; ia.m.len_strand = (const uint32_t*)(d_slot + 2 * np);
			ia.m.nfrag = ng / 2; ia.m.min_score = bm->min_score; ia.min_margin = bm->min_margin; ia.max_span = bm->max_span;
			ia.hist = (uint32_t*)(d_map + map_bytes); ia.counters = ia.hist + 3 * ((size_t)bm->max_span + 1);
			int wgs = c->dev_cus * 4;
			if (c->kn.istat_groups > 0) wgs = c->kn.istat_groups;
			uint32_t cnt[SSW_ISTAT_COUNTERS];
			if (ssw_shim_memset(ia.hist, 0, istat_bytes, c->stream)) { fail(c, "upload failed: %s", ssw_shim_last_error()); goto done; }
			ssw_shim_event_record(c->ev_a, c->stream);
			if (ssw_shim_launch_insertstat(&ia, wgs, c->stream)) { fail(c, "insertstat launch failed: %s", ssw_shim_last_error()); goto done; }
			ssw_shim_event_record(c->ev_b, c->stream);
			/* (hist is contiguous with the counters: the bins to the caller, the counters to the stack) */
			if (ssw_shim_d2h(bm->ihist, ia.hist, istat_bytes - sizeof cnt, c->stream) || ssw_shim_d2h(cnt, ia.counters, sizeof cnt, c->stream) ||
			    ssw_shim_stream_sync(c->stream)) { fail(c, "result download failed: %s", ssw_shim_last_error()); goto done; }
			ssw_gpu_insert_counts* ic = bm->icounts;
			ic->n_both = cnt[SSW_ISTAT_BOTH]; ic->n_unique = cnt[SSW_ISTAT_UNIQUE]; ic->n_same = cnt[SSW_ISTAT_SAME];
			for (int o = 0; o < 3; ++o) { ic->n_in[o] = cnt[SSW_ISTAT_IN + o]; ic->n_out[o] = cnt[SSW_ISTAT_OUT + o]; }
			c->tm.reduce_ms = ssw_shim_event_elapsed_ms(c->ev_a, c->ev_b);
			timing_add(&acc, &c->tm);
			acc.t.total_ms = wall_ms() - t_start;
			c->tm = acc.t;
			rc = 0;
			goto done;
		}
		ssw_shim_event_record(c->ev_a, c->stream);
		if (bm->mates) {
			ssw_matebest_args ma; memset(&ma, 0, sizeof ma);
			ma.rec = d_rec; ma.cand_off = d_off; ma.slot = d_slot; ma.tbeg = d_tbeg; ma.tidx = d_slot + np; ma.len_strand = (const uint32_t*)(d_slot + 2 * np);
			ma.nfrag = ng / 2; ma.min_score = bm->min_score; ma.min_insert = bm->min_insert; ma.max_insert = bm->max_insert;
			ma.unpaired_penalty = bm->unpaired_penalty; ma.orientation = bm->orientation;
			ma.ins_pen = bm->ins_pen ? (const uint16_t*)(d_map + map_bytes) : 0;
			ma.out = (struct ssw_out_rec*)d_sel; ma.sel = (struct ssw_mate_rec*)(d_sel + sizeof(struct ssw_out_rec) * (size_t)ng);
			if (ssw_shim_launch_matebest(&ma, c->stream)) { fail(c, "matebest launch failed: %s", ssw_shim_last_error()); goto done; }
			ssw_shim_event_record(c->ev_b, c->stream);
			if (ssw_shim_d2h(results, ma.out, sizeof(ssw_gpu_result) * (size_t)ng, c->stream) ||
			    ssw_shim_d2h(bm->mates, ma.sel, sizeof(ssw_gpu_mates) * (size_t)(ng / 2), c->stream) || ssw_shim_stream_sync(c->stream)) {
				fail(c, "result download failed: %s", ssw_shim_last_error()); goto done;
			}
		} else if (K) {
			ssw_grouptopk_args ta; memset(&ta, 0, sizeof ta);
			ta.rec = d_rec; ta.cand_off = d_off; ta.slot = d_slot; ta.ngroups = ng; ta.min_score = bm->min_score; ta.k = K; ta.max_drop = bm->max_drop;
			ta.out = (struct ssw_out_rec*)d_sel; ta.pos = (int32_t*)(d_sel + sizeof(struct ssw_out_rec) * (size_t)nout); ta.n_eligible = ta.pos + nout;
			if (ssw_shim_launch_grouptopk(&ta, c->stream)) { fail(c, "grouptopk launch failed: %s", ssw_shim_last_error()); goto done; }
			ssw_shim_event_record(c->ev_b, c->stream);
			if (ssw_shim_d2h(results, ta.out, sizeof(ssw_gpu_result) * (size_t)nout, c->stream) || ssw_shim_d2h(bm->pos, ta.pos, 4 * (size_t)nout, c->stream) ||
			    ssw_shim_d2h(bm->n_eligible, ta.n_eligible, 4 * (size_t)ng, c->stream) || ssw_shim_stream_sync(c->stream)) {
				fail(c, "result download failed: %s", ssw_shim_last_error()); goto done;
			}
		} else {
			ssw_groupbest_args ga; memset(&ga, 0, sizeof ga);
			ga.rec = d_rec; ga.cand_off = d_off; ga.slot = d_slot; ga.ngroups = ng; ga.min_score = bm->min_score;
			ga.out = (struct ssw_out_rec*)d_sel; ga.sel = (struct ssw_best_rec*)(d_sel + sizeof(struct ssw_out_rec) * (size_t)ng);
			if (ssw_shim_launch_groupbest(&ga, c->stream)) { fail(c, "groupbest launch failed: %s", ssw_shim_last_error()); goto done; }
			ssw_shim_event_record(c->ev_b, c->stream);
			if (ssw_shim_d2h(results, ga.out, sizeof(ssw_gpu_result) * (size_t)ng, c->stream) || ssw_shim_d2h(bm->sel, ga.sel, sizeof(ssw_gpu_best) * (size_t)ng, c->stream) ||
			    ssw_shim_stream_sync(c->stream)) { fail(c, "result download failed: %s", ssw_shim_last_error()); goto done; }
		}
		c->tm.reduce_ms = rescue_ms + ssw_shim_event_elapsed_ms(c->ev_a, c->ev_b);      /* (rescue_ms: k_materescue; 0 without a rescue stage) */
		/* ---- the winners alone go on: the fused path's through the reverse pass and the traceback (their fill records reused), the others
		   through the fallback once more with the caller's flag.  One survivor list over all output slots; top-k: every slot that holds a
		   candidate (pairs_flagged applies the reference's gate, and takes the fill's word mark out of the records it leaves alone) */
		int64_t nin = 0, nfw = 0, ngate = 0; int64_t* wg = 0;
		if (prm->flag != 0) {
			wlist = (int64_t*)malloc(sizeof(int64_t) * 2 * (size_t)nout); wrec = (ssw_gpu_result*)malloc(sizeof(ssw_gpu_result) * (size_t)nout);
			if (!wlist || !wrec) { fail(c, "out of host memory%s", ""); goto done; }
			const int64_t per = K ? K : 1;      /* output slots of a group */
			wg = wlist + nout;      /* wlist: the fused path's winners from the front, the fallback's from the back; wg: their output slots */
			for (int64_t g = 0; g < ng; ++g)
				for (int64_t o = g * per; o < (g + 1) * per; ++o) {
					const int32_t p = K ? bm->pos[o] : bm->mates ? (g & 1 ? bm->mates[g >> 1].pos2 : bm->mates[g >> 1].pos1) : bm->sel[g].best;
					if (p < 0) break;
					const int64_t i = bm->cand_off[g] + p;
					if (!(prm->flag == 2 && (int)results[o].score1 < prm->filters)) ++ngate;      /* ssw.c:916 */
					if (key[i] == PJ_KEY_FALLBACK) { ++nfw; wlist[nout - nfw] = i; wg[nout - nfw] = o; }
					else { wlist[nin] = i; wg[nin] = o; wrec[nin] = results[o]; ++nin; }
				}
			if (nin > 0 && pairs_flagged(c, Q, T, qidx, src, wlist, wrec, nin, prm, d_mat, maxmat, minmat, &st)) goto done;
			for (int64_t k = 0; k < nin; ++k) results[wg[k]] = wrec[k];
		}
		timing_add(&acc, &c->tm);
		if (nfw > 0) {
			if (best_fallback(c, Q, T, qidx, src, wlist + (nout - nfw), nfw, prm, wrec, &st, &acc)) goto done;
			for (int64_t k = 0; k < nfw; ++k) results[wg[nout - nfw + k]] = wrec[k];
		}
		acc.t.best_flagged = K ? ngate : nin + nfw;
	}
	if (!bm && nfb > 0 && (src->tbeg ? windows_fallback(c, Q, T, qidx, src, fb, nfb, prm, results, &st, &acc)
	                          : pairs_fallback(c, Q, T, qidx, tidx, fb, nfb, prm, results, &st, &acc))) goto done;
	if (st.n > 0) {      /* the pool in pair order (offsets as the caller's pool would have them, also when it asked for none) */
		uint32_t* pool = cigar_pool ? (uint32_t*)malloc(sizeof(uint32_t) * (size_t)st.n) : 0;
		if (cigar_pool && !pool) { fail(c, "out of host memory (%s)", "CIGAR pool"); goto done; }
		int64_t w = 0;
		for (int64_t i = 0; i < nout; ++i) {
			ssw_gpu_result* r = &results[i];
			if (r->cigarLen > 0 && r->cigar_off >= 0) {
				if (pool) memcpy(pool + w, st.words + r->cigar_off, sizeof(uint32_t) * (size_t)r->cigarLen);
				r->cigar_off = w; w += r->cigarLen;
			}
		}
		if (cigar_pool) *cigar_pool = pool;
		if (cigar_words) *cigar_words = w;
	}
	acc.t.rescue_windows = nresc;
	acc.t.total_ms = wall_ms() - t_start;
	c->tm = acc.t;
	rc = 0;
done:
	pair_fill_free(&pf); pair_fill_free(&pf2);
	free(key); free(st.words); free(slot); free(wlist); free(wrec); free(rlist);
	return rc;
}

static int align_pairs_locked(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int32_t* qidx, const int32_t* tidx,
                              int64_t np, const ssw_gpu_params* prm, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (np < 0 || (np > 0 && (!qidx || !tidx || !results))) return fail(c, "align_pairs: NULL argument%s", "");
	if (check_common(c, "align_pairs", Q, T, prm)) return -1;
	for (int64_t i = 0; i < np; ++i)
		if (qidx[i] < 0 || qidx[i] >= Q->count || tidx[i] < 0 || tidx[i] >= T->count) {
			char msg[160];
			snprintf(msg, sizeof msg, "pair %lld: query %d of %d, target %d of %d", (long long)i, qidx[i], Q->count, tidx[i], T->count);
			return fail(c, "align_pairs: index out of range (%s)", msg);
		}
	pair_src src; memset(&src, 0, sizeof src);
	src.tidx = tidx; src.who = "align_pairs";
	return pairs_core(c, Q, T, qidx, &src, np, prm, results, cigar_pool, cigar_words, 0);
}

int ssw_gpu_align_pairs(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int32_t* qidx, const int32_t* tidx, int64_t npairs,
                        const ssw_gpu_params* prm, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!c) return fail(0, "align_pairs: NULL context%s", "");
	if (ctx_enter(c, cigar_pool, cigar_words)) return SSW_GPU_BUSY;
	return ctx_leave(c, align_pairs_locked(c, Q, T, qidx, tidx, npairs, prm, results, cigar_pool, cigar_words));
}

/* ------------------------------------------------------------------------------------------------
 * Windows of resident targets (ssw_gpu_align_windows): pair i = query qidx[i] against columns [tbeg[i], tbeg[i] + tlen[i]) of target
 * tidx[i].  Inside the fused kernel's envelope nothing of the targets is copied: k_wintab turns the caller's three arrays into a device
 * table of (64-bit start, length), and k_fillpairs, the reverse pass, the traceback and k_mark read every window where it lies.
 * The windows outside the envelope are gathered on the device into temporary sets (identical windows once; a set holds at most
 * max(budget / 8, 1 MiB) residues, or one window) and go through the pair path: exact, slow.  win_copied counts their residues.
 * ------------------------------------------------------------------------------------------------ */
typedef struct { int32_t t, l; int64_t b, i; } wkey;
static int wkey_cmp(const void* pa, const void* pb)
{
	const wkey* a = (const wkey*)pa; const wkey* b = (const wkey*)pb;
	if (a->t != b->t) return a->t < b->t ? -1 : 1;
	if (a->b != b->b) return a->b < b->b ? -1 : 1;
	if (a->l != b->l) return a->l < b->l ? -1 : 1;
	return a->i < b->i ? -1 : a->i > b->i;
}

static int windows_fallback(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int32_t* qidx, const pair_src* src,
                            const int64_t* list, int64_t nl, const ssw_gpu_params* prm, ssw_gpu_result* results, cigar_stage* st, call_acc* acc)
{
	wkey* wk = (wkey*)malloc(sizeof(wkey) * (size_t)nl);
	int32_t* q2 = 0; int32_t* t2 = 0; int32_t* gidx = 0; int64_t* gbeg = 0; int64_t* goff = 0; ssw_gpu_result* tmp = 0;
	int rc = -1;
	if (!wk) { fail(c, "out of host memory%s", ""); goto out; }
	for (int64_t k = 0; k < nl; ++k) { const int64_t i = list[k]; wk[k].t = src->tidx[i]; wk[k].b = src->tbeg[i]; wk[k].l = src->tlen[i]; wk[k].i = i; }
	qsort(wk, (size_t)nl, sizeof(wkey), wkey_cmp);
	int64_t lim = (int64_t)(c->cm_budget / 8); if (lim < ((int64_t)1 << 20)) lim = (int64_t)1 << 20;
	for (int64_t k0 = 0; k0 < nl; ) {
		/* a chunk: the pairs of consecutive distinct windows whose residues stay within `lim` (one window at the least) */
		int64_t k1 = k0, nd = 0, sum = 0;
		while (k1 < nl) {
			int64_t e = k1 + 1;
			while (e < nl && wk[e].t == wk[k1].t && wk[e].b == wk[k1].b && wk[e].l == wk[k1].l) ++e;
			if (nd > 0 && (sum + wk[k1].l > lim || nd >= 0x7fffff00 || e - k0 > 0x7fffff00)) break;
			sum += wk[k1].l; ++nd; k1 = e;
		}
		const int64_t m = k1 - k0;
		if (m > 0x7fffffff) { fail(c, "align_windows: %s", "more than 2^31 pairs against one window outside the fused kernel's envelope"); goto out; }
		free(q2); free(gidx); free(gbeg); free(goff); free(tmp);
		q2 = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)m); t2 = q2 ? q2 + m : 0;
		gidx = (int32_t*)malloc(sizeof(int32_t) * (size_t)nd); gbeg = (int64_t*)malloc(sizeof(int64_t) * (size_t)nd);
		goff = (int64_t*)malloc(sizeof(int64_t) * ((size_t)nd + 1)); tmp = (ssw_gpu_result*)malloc(sizeof(ssw_gpu_result) * (size_t)m);
		if (!q2 || !gidx || !gbeg || !goff || !tmp) { fail(c, "out of host memory%s", ""); goto out; }
		int64_t d = -1;
		goff[0] = 0;
		for (int64_t k = k0; k < k1; ++k) {
			if (k == k0 || wk[k].t != wk[k - 1].t || wk[k].b != wk[k - 1].b || wk[k].l != wk[k - 1].l) {
				++d; gidx[d] = wk[k].t; gbeg[d] = wk[k].b; goff[d + 1] = goff[d] + wk[k].l;
			}
			q2[k - k0] = qidx[wk[k].i]; t2[k - k0] = (int32_t)d;
		}
		ssw_gpu_seqs* G = seqs_new(c, goff, (int32_t)nd);
		if (!G) goto out;
		G->codes_ranged = T->codes_ranged; G->code_lo = T->code_lo; G->code_hi = T->code_hi;      /* windows of T */
		unsigned char* d_g = (unsigned char*)ssw_shim_malloc(12 * (size_t)nd);
		ssw_seqgather_args ga; memset(&ga, 0, sizeof ga);
		ga.src = T->d_codes; ga.src_off = T->d_off; ga.src_beg = (const int64_t*)d_g; ga.idx = (const int32_t*)(d_g + 8 * (size_t)nd);
		ga.dst_off = G->d_off; ga.dst = G->d_codes; ga.count = (int32_t)nd;
		const int ok = d_g && !ssw_shim_h2d((void*)ga.src_beg, gbeg, 8 * (size_t)nd, c->stream) && !ssw_shim_h2d((void*)ga.idx, gidx, 4 * (size_t)nd, c->stream) &&
		               !ssw_shim_h2d(G->d_off, G->h_off, sizeof(int64_t) * ((size_t)nd + 1), c->stream) &&
		               !ssw_shim_launch_seqgather(&ga, c->stream) && !ssw_shim_stream_sync(c->stream);
		ssw_shim_free(d_g);
		if (!ok) { fail(c, "align_windows: window gather failed: %s", ssw_shim_last_error()); ssw_gpu_seqs_free(G); goto out; }
		uint32_t* pool = 0; int64_t words = 0;
		if (align_pairs_locked(c, Q, G, q2, t2, m, prm, tmp, &pool, &words)) { ssw_gpu_seqs_free(G); goto out; }
		ssw_gpu_seqs_free(G);
		timing_add(acc, &c->tm);
		acc->t.win_copied += sum;
		if (stage_append_batch(c, st, pool, words, tmp, m, &wk[k0].i, sizeof(wkey), results)) goto out;
		k0 = k1;
	}
	rc = 0;
out:
	free(wk); free(q2); free(gidx); free(gbeg); free(goff); free(tmp);
	return rc;
}

/* every pair's indices and window inside its target, or -1 with a message that names the first pair that is not */
static int windows_check(ssw_gpu_ctx* c, const char* who, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int32_t* qidx, const int32_t* tidx,
                         const int64_t* tbeg, const int32_t* tlen, int64_t np)
{
	for (int64_t i = 0; i < np; ++i) {
		char msg[240];
		if (qidx[i] < 0 || qidx[i] >= Q->count || tidx[i] < 0 || tidx[i] >= T->count) {
			snprintf(msg, sizeof msg, "%s: index out of range (pair %lld: query %d of %d, target %d of %d)", who, (long long)i, qidx[i], Q->count, tidx[i], T->count);
			return fail(c, "%s", msg);
		}
		const int64_t tl = T->h_off[tidx[i] + 1] - T->h_off[tidx[i]];
		if (tbeg[i] < 0 || tlen[i] < 0 || tbeg[i] > tl || (int64_t)tlen[i] > tl - tbeg[i]) {      /* no clamping: a window that leaves its target is the caller's bug */
			snprintf(msg, sizeof msg, "%s: window out of range (pair %lld: columns [%lld, %lld + %d) of target %d, which has %lld)", who, (long long)i,
			         (long long)tbeg[i], (long long)tbeg[i], tlen[i], tidx[i], (long long)tl);
			return fail(c, "%s", msg);
		}
	}
	return 0;
}

static int align_windows_locked(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int32_t* qidx, const int32_t* tidx,
                                const int64_t* tbeg, const int32_t* tlen, int64_t np, const ssw_gpu_params* prm, ssw_gpu_result* results,
                                uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (np < 0 || (np > 0 && (!qidx || !tidx || !tbeg || !tlen || !results))) return fail(c, "align_windows: NULL argument%s", "");
	if (check_common(c, "align_windows", Q, T, prm)) return -1;
	if (np > 0x7fffff00) return fail(c, "align_windows: %s", "more than 2^31 pairs in one call");      /* (a pair's window is named by a 32-bit index) */
	if (windows_check(c, "align_windows", Q, T, qidx, tidx, tbeg, tlen, np)) return -1;
	pair_src src; memset(&src, 0, sizeof src);
	src.tidx = tidx; src.tbeg = tbeg; src.tlen = tlen; src.who = "align_windows";
	return pairs_core(c, Q, T, qidx, &src, np, prm, results, cigar_pool, cigar_words, 0);
}

int ssw_gpu_align_windows(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int32_t* qidx, const int32_t* tidx,
                          const int64_t* tbeg, const int32_t* tlen, int64_t npairs, const ssw_gpu_params* prm, ssw_gpu_result* results,
                          uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!c) return fail(0, "align_windows: NULL context%s", "");
	if (ctx_enter(c, cigar_pool, cigar_words)) return SSW_GPU_BUSY;
	return ctx_leave(c, align_windows_locked(c, Q, T, qidx, tidx, tbeg, tlen, npairs, prm, results, cigar_pool, cigar_words));
}

/* ------------------------------------------------------------------------------------------------
 * Best candidate window per read (ssw_gpu_align_windows_best): ssw_gpu_align_windows' pair list in groups, pairs_core in select mode.
 * ------------------------------------------------------------------------------------------------ */
static int align_windows_best_locked(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int64_t* cand_off, int64_t ng,
                                     const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen, const ssw_gpu_params* prm,
                                     int32_t min_score, ssw_gpu_best* sel, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words)
{
	char msg[200];
	if (cigar_pool) *cigar_pool = 0;      /* (this entry point alone empties its pool outputs before the argument checks) */
	if (cigar_words) *cigar_words = 0;
	if (ng < 0 || (ng > 0 && (!cand_off || !sel || !results))) return fail(c, "align_windows_best: NULL argument%s", "");
	if (check_common(c, "align_windows_best", Q, T, prm)) return -1;
	if (ng == 0) { memset(&c->tm, 0, sizeof c->tm); return 0; }
	if (cand_off[0] != 0) {
		snprintf(msg, sizeof msg, "group 0 starts at candidate %lld", (long long)cand_off[0]);
		return fail(c, "align_windows_best: cand_off[0] must be 0 (%s)", msg);
	}
	for (int64_t g = 0; g < ng; ++g)
		if (cand_off[g + 1] < cand_off[g]) {
			snprintf(msg, sizeof msg, "group %lld: candidates [%lld, %lld)", (long long)g, (long long)cand_off[g], (long long)cand_off[g + 1]);
			return fail(c, "align_windows_best: cand_off decreases (%s)", msg);
		}
	const int64_t np = cand_off[ng];
	if (np > 0x7fffff00) return fail(c, "align_windows_best: %s", "more than 2^31 candidates in one call");
	if (np > 0 && (!qidx || !tidx || !tbeg || !tlen)) return fail(c, "align_windows_best: NULL argument%s", "");
	if (windows_check(c, "align_windows_best", Q, T, qidx, tidx, tbeg, tlen, np)) return -1;
	if (np == 0) {      /* empty groups only */
		memset(&c->tm, 0, sizeof c->tm);
		for (int64_t g = 0; g < ng; ++g) { topk_pad(&results[g]); sel[g].best = sel[g].second = -1; sel[g].n_eligible = 0; sel[g].second_score1 = 0; sel[g].pad = 0; }
		return 0;
	}
	pair_src src; memset(&src, 0, sizeof src);
	src.tidx = tidx; src.tbeg = tbeg; src.tlen = tlen; src.who = "align_windows_best";
	best_mode bm; memset(&bm, 0, sizeof bm);
	bm.cand_off = cand_off; bm.ngroups = ng; bm.min_score = min_score; bm.sel = sel;
	return pairs_core(c, Q, T, qidx, &src, np, prm, results, cigar_pool, cigar_words, &bm);
}

int ssw_gpu_align_windows_best(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int64_t* cand_off, int64_t ngroups,
                               const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                               const ssw_gpu_params* prm, int32_t min_score, ssw_gpu_best* sel, ssw_gpu_result* results,
                               uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!c) return fail(0, "align_windows_best: NULL context%s", "");
	if (ctx_enter(c, cigar_pool, cigar_words)) return SSW_GPU_BUSY;
	return ctx_leave(c, align_windows_best_locked(c, Q, T, cand_off, ngroups, qidx, tidx, tbeg, tlen, prm, min_score, sel, results, cigar_pool, cigar_words));
}

/* ------------------------------------------------------------------------------------------------
 * Best candidate pair per read pair (ssw_gpu_align_windows_mates): the same select mode over 2 * nfrag groups, the selection per FRAGMENT
 * (k_matebest).  Device state that outlives a fill launch, an input / output of the call like the window table: per candidate 48 bytes of
 * record, 4 of slot map and 16 of side table (tbeg, tidx, read length | strand), per fragment 128 bytes of output (two records, one
 * selection) and 16 of offsets; under a pair model (ssw_gpu_align_windows_mates_model) the penalty table, 2 bytes per entry, behind the side
 * table.
 * ------------------------------------------------------------------------------------------------ */
static void mates_pad(ssw_gpu_mates* m) { memset(m, 0, sizeof *m); m->pos1 = m->pos2 = -1; }

/* "<who>: <what> (<detail>)" */
static int fail_who_d(ssw_gpu_ctx* c, const char* who, const char* what, const char* detail)
{
	char msg[400];
	snprintf(msg, sizeof msg, "%s: %s (%s)", who, what, detail);
	return fail(c, "%s", msg);
}

/* the argument checks of ssw_gpu_align_windows_mates_lib, shared with the rescue entry point: -1 refused (message written), 1 no fragments
   (nothing to do), 0 go on with *np_out candidates */
static int mates_check(ssw_gpu_ctx* c, const char* who, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int64_t* cand_off, int64_t nf,
                       const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen, int32_t nfwd,
                       const ssw_gpu_params* prm, int32_t min_insert, int32_t max_insert, int32_t unpaired_penalty, int32_t orientation,
                       const void* sel, const void* results, int64_t* np_out)
{
	char msg[200];
	if (nf < 0 || (nf > 0 && (!cand_off || !sel || !results))) return fail_who(c, who, "NULL argument");
	if (check_common(c, who, Q, T, prm)) return -1;
	if (nf == 0) { memset(&c->tm, 0, sizeof c->tm); return 1; }
	if (nf > 0x7fffff00 / 2) {
		snprintf(msg, sizeof msg, "%lld fragments", (long long)nf);
		return fail_who_d(c, who, "more than 2^31 output slots in one call", msg);
	}
	if (min_insert < 0 || min_insert > max_insert) {
		snprintf(msg, sizeof msg, "min_insert = %d, max_insert = %d", min_insert, max_insert);
		return fail_who_d(c, who, "0 <= min_insert <= max_insert required", msg);
	}
	if (unpaired_penalty < 0 || unpaired_penalty > 65535) {
		snprintf(msg, sizeof msg, "unpaired_penalty = %d", unpaired_penalty);
		return fail_who_d(c, who, "unpaired_penalty must be 0 .. 65535", msg);
	}
	if (orientation < SSW_GPU_MATES_FR || orientation > SSW_GPU_MATES_FF) {
		snprintf(msg, sizeof msg, "orientation = %d", orientation);
		return fail_who_d(c, who, "orientation must be SSW_GPU_MATES_FR, _RF or _FF", msg);
	}
	if (nfwd < 0 || nfwd > Q->count) {
		snprintf(msg, sizeof msg, "nfwd = %d, %d queries", nfwd, Q->count);
		return fail_who_d(c, who, "nfwd outside the query set", msg);
	}
	if (cand_off[0] != 0) {
		snprintf(msg, sizeof msg, "fragment 0 starts at candidate %lld", (long long)cand_off[0]);
		return fail_who_d(c, who, "cand_off[0] must be 0", msg);
	}
	const int64_t ng = 2 * nf;
	for (int64_t g = 0; g < ng; ++g) {
		const int64_t sz = cand_off[g + 1] - cand_off[g];
		if (sz >= 0 && sz <= SSW_GPU_MATES_GROUP_MAX) continue;
		snprintf(msg, sizeof msg, "fragment %lld, mate %d: candidates [%lld, %lld)", (long long)(g >> 1), (int)(g & 1) + 1, (long long)cand_off[g], (long long)cand_off[g + 1]);
		return fail_who_d(c, who, sz < 0 ? "cand_off decreases" : "more than 4096 candidates in a group", msg);
	}
	const int64_t np = cand_off[ng];
	if (np > 0x7fffff00) return fail_who(c, who, "more than 2^31 candidates in one call");
	if (np > 0 && (!qidx || !tidx || !tbeg || !tlen)) return fail_who(c, who, "NULL argument");
	if (windows_check(c, who, Q, T, qidx, tidx, tbeg, tlen, np)) return -1;
	*np_out = np;
	return 0;
}

/* the pair model's own refusals, after mates_check's (min_insert <= max_insert holds): a table over more than SSW_GPU_INSERT_TABLE_MAX spans */
static int model_check(ssw_gpu_ctx* c, const char* who, int32_t min_insert, int32_t max_insert, const uint16_t* ins_pen)
{
	const int64_t n_ins = (int64_t)max_insert - min_insert + 1;
	if (!ins_pen || n_ins <= SSW_GPU_INSERT_TABLE_MAX) return 0;
	char msg[200];
	snprintf(msg, sizeof msg, "min_insert = %d, max_insert = %d: %lld entries", min_insert, max_insert, (long long)n_ins);
	return fail_who_d(c, who, "insert_penalty covers more than 65536 spans", msg);
}

/* (who: the entry point's name in messages; ins_pen: the pair model's table or NULL -- ssw_gpu_align_windows_mates_lib is the NULL case) */
static int align_windows_mates_locked(ssw_gpu_ctx* c, const char* who, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int64_t* cand_off, int64_t nf,
                                      const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen, int32_t nfwd,
                                      const ssw_gpu_params* prm, int32_t min_score, int32_t min_insert, int32_t max_insert, int32_t unpaired_penalty,
                                      int32_t orientation, const uint16_t* ins_pen, ssw_gpu_mates* sel, ssw_gpu_result* results, uint32_t** cigar_pool,
                                      int64_t* cigar_words)
{
	if (cigar_pool) *cigar_pool = 0;      /* (as ssw_gpu_align_windows_best: the pool outputs are emptied before the argument checks) */
	if (cigar_words) *cigar_words = 0;
	int64_t np = 0;
	const int chk = mates_check(c, who, Q, T, cand_off, nf, qidx, tidx, tbeg, tlen, nfwd, prm, min_insert, max_insert, unpaired_penalty,
	                            orientation, sel, results, &np);
	if (chk < 0) return -1;
	if (model_check(c, who, min_insert, max_insert, ins_pen)) return -1;
	if (chk) return 0;
	const int64_t ng = 2 * nf;
	if (np == 0) {      /* empty groups only */
		memset(&c->tm, 0, sizeof c->tm);
		for (int64_t g = 0; g < ng; ++g) topk_pad(&results[g]);
		for (int64_t f = 0; f < nf; ++f) mates_pad(&sel[f]);
		return 0;
	}
	pair_src src; memset(&src, 0, sizeof src);
	src.tidx = tidx; src.tbeg = tbeg; src.tlen = tlen; src.who = who;
	best_mode bm; memset(&bm, 0, sizeof bm);
	bm.cand_off = cand_off; bm.ngroups = ng; bm.min_score = min_score; bm.mates = sel;
	bm.nfwd = nfwd; bm.min_insert = min_insert; bm.max_insert = max_insert; bm.unpaired_penalty = unpaired_penalty;
	bm.orientation = orientation; bm.ins_pen = ins_pen; bm.n_ins = (int64_t)max_insert - min_insert + 1;
	return pairs_core(c, Q, T, qidx, &src, np, prm, results, cigar_pool, cigar_words, &bm);
}

int ssw_gpu_align_windows_mates_lib(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int64_t* cand_off, int64_t nfrag,
                                    const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen, int32_t nfwd,
                                    const ssw_gpu_params* prm, int32_t min_score, int32_t min_insert, int32_t max_insert, int32_t unpaired_penalty,
                                    int32_t orientation, ssw_gpu_mates* sel, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!c) return fail(0, "align_windows_mates: NULL context%s", "");
	if (ctx_enter(c, cigar_pool, cigar_words)) return SSW_GPU_BUSY;
	return ctx_leave(c, align_windows_mates_locked(c, "align_windows_mates", Q, T, cand_off, nfrag, qidx, tidx, tbeg, tlen, nfwd, prm, min_score, min_insert,
	                                               max_insert, unpaired_penalty, orientation, 0, sel, results, cigar_pool, cigar_words));
}

/* ssw_gpu_align_windows_mates_lib under a pair model: the four pairing arguments in one struct, and a penalty per span of a proper combination */
int ssw_gpu_align_windows_mates_model(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int64_t* cand_off, int64_t nfrag,
                                      const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen, int32_t nfwd,
                                      const ssw_gpu_params* prm, int32_t min_score, const ssw_gpu_pair_model* model,
                                      ssw_gpu_mates* sel, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words)
{
	static const char who[] = "align_windows_mates_model";
	if (!c) return fail(0, "%s: NULL context", who);
	if (ctx_enter(c, cigar_pool, cigar_words)) return SSW_GPU_BUSY;
	if (!model) {      /* (the pool outputs are emptied as by every other refusal) */
		if (cigar_pool) *cigar_pool = 0;
		if (cigar_words) *cigar_words = 0;
		return ctx_leave(c, fail_who_d(c, who, "NULL argument", "model"));
	}
	return ctx_leave(c, align_windows_mates_locked(c, who, Q, T, cand_off, nfrag, qidx, tidx, tbeg, tlen, nfwd, prm, min_score, model->min_insert,
	                                               model->max_insert, model->unpaired_penalty, model->orientation, model->insert_penalty, sel, results,
	                                               cigar_pool, cigar_words));
}

int ssw_gpu_align_windows_mates(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int64_t* cand_off, int64_t nfrag,
                                const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen, int32_t nfwd,
                                const ssw_gpu_params* prm, int32_t min_score, int32_t min_insert, int32_t max_insert, int32_t unpaired_penalty,
                                ssw_gpu_mates* sel, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words)
{
	return ssw_gpu_align_windows_mates_lib(c, Q, T, cand_off, nfrag, qidx, tidx, tbeg, tlen, nfwd, prm, min_score, min_insert, max_insert,
	                                       unpaired_penalty, SSW_GPU_MATES_FR, sel, results, cigar_pool, cigar_words);
}

/* ------------------------------------------------------------------------------------------------
 * Insert-size histogram (ssw_gpu_insert_hist): the mates call's groups, checks, fill and side table at flag 0, k_insertstat in place of the
 * selection.  Device state beyond the fill's records, the slot map and the side table: 3 * (max_span + 1) bins and 16 counters, 32-bit,
 * behind the side table (at most 768 KiB + 64 bytes); nothing per fragment comes to the host.
 * ------------------------------------------------------------------------------------------------ */
static int insert_hist_locked(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int64_t* cand_off, int64_t nf,
                              const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen, int32_t nfwd,
                              const ssw_gpu_params* prm, int32_t min_score, int32_t min_margin, int32_t max_span, uint32_t* hist,
                              ssw_gpu_insert_counts* counts)
{
	static const char who[] = "insert_hist";
	char msg[120];
	if (!hist || !counts) return fail_who(c, who, "NULL argument");
	/* the fill is flag 0's whatever the caller's record says: flag, filters, filterd and mark_mismatch are not looked at */
	ssw_gpu_params p0; memset(&p0, 0, sizeof p0);
	if (prm) { p0 = *prm; p0.flag = 0; p0.filters = 0; p0.filterd = 0; p0.mark_mismatch = 0; }
	int64_t np = 0;
	const int chk = mates_check(c, who, Q, T, cand_off, nf, qidx, tidx, tbeg, tlen, nfwd, prm ? &p0 : 0, 0, 0, 0, SSW_GPU_MATES_FR, hist, counts, &np);
	if (chk < 0) return -1;
	if (min_margin < 0 || min_margin > 65535) {
		snprintf(msg, sizeof msg, "min_margin = %d", min_margin);
		return fail_who_d(c, who, "min_margin must be 0 .. 65535", msg);
	}
	if (max_span < 0 || max_span > SSW_GPU_INSERT_SPAN_MAX) {
		snprintf(msg, sizeof msg, "max_span = %d", max_span);
		return fail_who_d(c, who, "max_span must be 0 .. 65535", msg);
	}
	memset(hist, 0, sizeof(uint32_t) * 3 * ((size_t)max_span + 1));
	memset(counts, 0, sizeof *counts);
	if (chk || np == 0) { memset(&c->tm, 0, sizeof c->tm); return 0; }      /* no fragments, or empty groups only */
	pair_src src; memset(&src, 0, sizeof src);
	src.tidx = tidx; src.tbeg = tbeg; src.tlen = tlen; src.who = who;
	best_mode bm; memset(&bm, 0, sizeof bm);
	bm.cand_off = cand_off; bm.ngroups = 2 * nf; bm.min_score = min_score; bm.nfwd = nfwd;
	bm.ihist = hist; bm.icounts = counts; bm.min_margin = min_margin; bm.max_span = max_span;
	return pairs_core(c, Q, T, qidx, &src, np, &p0, 0, 0, 0, &bm);
}

int ssw_gpu_insert_hist(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int64_t* cand_off, int64_t nfrag,
                        const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen, int32_t nfwd,
                        const ssw_gpu_params* prm, int32_t min_score, int32_t min_margin, int32_t max_span, uint32_t* hist,
                        ssw_gpu_insert_counts* counts)
{
	if (!c) return fail(0, "insert_hist: NULL context%s", "");
	if (ctx_enter(c, 0, 0)) return SSW_GPU_BUSY;
	return ctx_leave(c, insert_hist_locked(c, Q, T, cand_off, nfrag, qidx, tidx, tbeg, tlen, nfwd, prm, min_score, min_margin, max_span, hist, counts));
}

/* ------------------------------------------------------------------------------------------------
 * ssw_gpu_insert_fit: quartiles, outlier bounds, mean and standard deviation of one histogram row and the insert range they give (the
 * rule of BWA-MEM's mem_pestat, the rounding pinned in integers).  Host arithmetic only.  Every floating-point operation is one
 * correctly rounded IEEE operation on doubles -- no contraction into fused multiply-adds --, and n * S2 - S1 * S1 is formed exactly in
 * 128 bits and converted ONCE, so that mean and sd are the same bits on every host.
 * ------------------------------------------------------------------------------------------------ */
static int32_t fit_kth(const uint32_t* h, int32_t ne, int64_t k)      /* k-th smallest span, 0-based: the smallest d with h[0] + .. + h[d] > k */
{
	int64_t run = 0;
	for (int32_t d = 0; d < ne; ++d) { run += h[d]; if (run > k) return d; }
	return ne - 1;
}
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))      /* (gcc has no FP_CONTRACT pragma) */
#endif
int ssw_gpu_insert_fit(const uint32_t* h, int32_t ne, ssw_gpu_insert_stats* out)
{
#ifdef __clang__
#pragma STDC FP_CONTRACT OFF
#endif
	if (!h || !out || ne < 1) return -1;
	int64_t N = 0;
	for (int32_t d = 0; d < ne; ++d) { N += h[d]; if (N >= ((int64_t)1 << 31)) return -1; }
	memset(out, 0, sizeof *out);
	out->n_total = N;
	if (N < 10) return 1;
	const int32_t p25 = fit_kth(h, ne, (250 * N + 499) / 1000), p50 = fit_kth(h, ne, (500 * N + 499) / 1000), p75 = fit_kth(h, ne, (750 * N + 499) / 1000);
	const int64_t iqr = (int64_t)p75 - p25;
	int64_t lo = p25 - 2 * iqr, hi = p75 + 2 * iqr;
	if (lo < 1) lo = 1;
	if (hi > ne - 1) hi = ne - 1;
	uint64_t n = 0, S1 = 0;      /* (n < 2^31, d < 2^31: S1 < 2^62, S2 < 2^93) */
	unsigned __int128 S2 = 0;
	for (int64_t d = lo; d <= hi; ++d) { n += h[d]; S1 += (uint64_t)d * h[d]; S2 += (unsigned __int128)((uint64_t)d * (uint64_t)d) * h[d]; }
	if (n == 0) return 1;
	const unsigned __int128 num = (unsigned __int128)n * S2 - (unsigned __int128)S1 * S1;      /* n^2 x variance >= 0 (Cauchy-Schwarz) */
	const double mean = (double)S1 / (double)n;
	const double sd = sqrt((double)num / ((double)n * (double)n));
	int64_t low = (int64_t)floor(mean - 4.0 * sd + 0.499), high = (int64_t)floor(mean + 4.0 * sd + 0.499);
	if (p25 - 3 * iqr < low) low = p25 - 3 * iqr;
	if (p75 + 3 * iqr > high) high = p75 + 3 * iqr;
	out->n_used = (int64_t)n;
	out->p25 = p25; out->p50 = p50; out->p75 = p75;
	out->out_lo = (int32_t)lo; out->out_hi = (int32_t)hi;
	out->sum = S1; out->sum2 = (uint64_t)S2;      /* (S2 fits for n_entries <= 65536) */
	out->mean = mean; out->sd = sd;
	out->min_insert = (int32_t)(low > 1 ? low : 1);
	out->max_insert = (int32_t)(high < ne - 1 ? high : ne - 1);
	return 0;
}

/* ------------------------------------------------------------------------------------------------
 * Mate rescue (ssw_gpu_align_windows_mates_rescue): ssw_gpu_align_windows_mates_lib over the AUGMENTED list -- every group followed by
 * max_anchors rescue slots, which k_materescue fills on the device from the other mate's best candidates (pairs_core's rescue stage).
 * The augmented list is built here, with the slots empty; pairs_core enters the windows of the non-empty ones.  Device state beyond
 * the mates call's: 24 bytes per slot, 4 of mate_q per group, and the records and maps of the slots like any other candidate's.
 * ------------------------------------------------------------------------------------------------ */
static int align_windows_mates_rescue_locked(ssw_gpu_ctx* c, const char* who, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int64_t* cand_off,
                                             int64_t nf, const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen, int32_t nfwd,
                                             const int32_t* mate_q, const ssw_gpu_params* prm, int32_t min_score, int32_t min_insert, int32_t max_insert,
                                             int32_t unpaired_penalty, int32_t orientation, const uint16_t* ins_pen, int32_t max_anchors,
                                             int32_t anchor_min_score, int32_t rescue_pad, ssw_gpu_mates* sel, ssw_gpu_result* results,
                                             ssw_gpu_rescued* origin, uint32_t** cigar_pool, int64_t* cigar_words)
{
	char msg[240];
	if (cigar_pool) *cigar_pool = 0;
	if (cigar_words) *cigar_words = 0;
	int64_t np = 0;
	const int chk = mates_check(c, who, Q, T, cand_off, nf, qidx, tidx, tbeg, tlen, nfwd, prm, min_insert, max_insert, unpaired_penalty, orientation,
	                            sel, results, &np);
	if (chk < 0) return -1;
	if (model_check(c, who, min_insert, max_insert, ins_pen)) return -1;
	if (chk) return 0;
	if (!mate_q || !origin) return fail_who(c, who, "NULL argument");
	if ((int64_t)Q->count != 2 * (int64_t)nfwd) {
		snprintf(msg, sizeof msg, "nfwd = %d, %d queries", nfwd, Q->count);
		return fail_who_d(c, who, "queries->count must be 2 * nfwd, the reverse complements resident", msg);
	}
	if (max_anchors < 1 || max_anchors > SSW_GPU_RESCUE_ANCHORS_MAX) {
		snprintf(msg, sizeof msg, "max_anchors = %d", max_anchors);
		return fail_who_d(c, who, "max_anchors must be 1 .. 8", msg);
	}
	if (rescue_pad < 0 || rescue_pad > 65535) {
		snprintf(msg, sizeof msg, "rescue_pad = %d", rescue_pad);
		return fail_who_d(c, who, "rescue_pad must be 0 .. 65535", msg);
	}
	if (anchor_min_score < 0) {
		snprintf(msg, sizeof msg, "anchor_min_score = %d", anchor_min_score);
		return fail_who_d(c, who, "anchor_min_score must be >= 0", msg);
	}
	const int64_t ng = 2 * nf, A = max_anchors;
	for (int64_t g = 0; g < ng; ++g) {
		const int64_t sz = cand_off[g + 1] - cand_off[g];
		if (mate_q[g] < 0 || mate_q[g] >= nfwd) {
			snprintf(msg, sizeof msg, "fragment %lld, mate %d: mate_q = %d, nfwd = %d", (long long)(g >> 1), (int)(g & 1) + 1, mate_q[g], nfwd);
			return fail_who_d(c, who, "mate_q outside the forward reads", msg);
		}
		if (sz + A > SSW_GPU_MATES_GROUP_MAX) {
			snprintf(msg, sizeof msg, "fragment %lld, mate %d: %lld candidates + %d rescue slots", (long long)(g >> 1), (int)(g & 1) + 1, (long long)sz, max_anchors);
			return fail_who_d(c, who, "more than 4096 candidates and rescue slots in a group", msg);
		}
		for (int64_t i = cand_off[g]; i < cand_off[g + 1]; ++i)
			if (qidx[i] != mate_q[g] && qidx[i] != nfwd + mate_q[g]) {
				snprintf(msg, sizeof msg, "pair %lld of fragment %lld, mate %d: query %d, mate_q = %d, nfwd = %d", (long long)i, (long long)(g >> 1), (int)(g & 1) + 1,
				         qidx[i], mate_q[g], nfwd);
				return fail_who_d(c, who, "a candidate's query is neither strand of its mate's read", msg);
			}
	}
	const int64_t npa = np + ng * A;
	if (npa > 0x7fffff00) return fail_who(c, who, "more than 2^31 candidates and rescue slots in one call");
	/* the augmented list: group g = the caller's candidates, then A empty slots (tlen 0) on the mate's forward read */
	int64_t* off_a = (int64_t*)malloc(sizeof(int64_t) * ((size_t)ng + 1 + (size_t)npa));
	int32_t* q_a = (int32_t*)malloc(sizeof(int32_t) * 3 * (size_t)npa);
	ssw_gpu_rescued* slots = (ssw_gpu_rescued*)malloc(sizeof(ssw_gpu_rescued) * (size_t)(ng * A));
	int rc = -1;
	if (!off_a || !q_a || !slots) { fail(c, "out of host memory%s", ""); goto out; }
	int64_t* b_a = off_a + ng + 1; int32_t* t_a = q_a + npa; int32_t* l_a = q_a + 2 * npa;
	off_a[0] = 0;
	for (int64_t g = 0; g < ng; ++g) {
		const int64_t c0 = cand_off[g], sz = cand_off[g + 1] - c0, a0 = off_a[g];
		if (sz > 0) {
			memcpy(q_a + a0, qidx + c0, sizeof(int32_t) * (size_t)sz); memcpy(t_a + a0, tidx + c0, sizeof(int32_t) * (size_t)sz);
			memcpy(b_a + a0, tbeg + c0, sizeof(int64_t) * (size_t)sz); memcpy(l_a + a0, tlen + c0, sizeof(int32_t) * (size_t)sz);
		}
		for (int64_t i = a0 + sz; i < a0 + sz + A; ++i) { q_a[i] = mate_q[g]; t_a[i] = 0; b_a[i] = 0; l_a[i] = 0; }
		off_a[g + 1] = a0 + sz + A;
	}
	pair_src src; memset(&src, 0, sizeof src);
	src.tidx = t_a; src.tbeg = b_a; src.tlen = l_a; src.who = who;
	best_mode bm; memset(&bm, 0, sizeof bm);
	bm.cand_off = off_a; bm.ngroups = ng; bm.min_score = min_score; bm.mates = sel;
	bm.nfwd = nfwd; bm.min_insert = min_insert; bm.max_insert = max_insert; bm.unpaired_penalty = unpaired_penalty;
	bm.orientation = orientation; bm.ins_pen = ins_pen; bm.n_ins = (int64_t)max_insert - min_insert + 1;
	bm.rescue_anchors = max_anchors; bm.anchor_min_score = anchor_min_score; bm.rescue_pad = rescue_pad; bm.mate_q = mate_q;
	bm.r_qidx = q_a; bm.r_tidx = t_a; bm.r_tbeg = b_a; bm.r_tlen = l_a; bm.r_slots = slots;
	rc = pairs_core(c, Q, T, q_a, &src, npa, prm, results, cigar_pool, cigar_words, &bm);
	if (rc == 0)
		for (int64_t g = 0; g < ng; ++g) {
			const int32_t pos = g & 1 ? sel[g >> 1].pos2 : sel[g >> 1].pos1;
			ssw_gpu_rescued* o = &origin[g];
			if (pos < 0) { o->tbeg = 0; o->tlen = 0; o->tidx = -1; o->qidx = -1; o->anchor = -1; continue; }
			const int64_t i = off_a[g] + pos, sz = cand_off[g + 1] - cand_off[g];
			o->tbeg = b_a[i]; o->tlen = l_a[i]; o->tidx = t_a[i]; o->qidx = q_a[i];
			o->anchor = pos >= sz ? slots[g * A + (pos - sz)].anchor : -1;
		}
out:
	free(off_a); free(q_a); free(slots);
	return rc;
}

int ssw_gpu_align_windows_mates_rescue(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int64_t* cand_off, int64_t nfrag,
                                       const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen, int32_t nfwd,
                                       const int32_t* mate_q, const ssw_gpu_params* prm, int32_t min_score, int32_t min_insert, int32_t max_insert,
                                       int32_t unpaired_penalty, int32_t orientation, int32_t max_anchors, int32_t anchor_min_score, int32_t rescue_pad,
                                       ssw_gpu_mates* sel, ssw_gpu_result* results, ssw_gpu_rescued* origin, uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!c) return fail(0, "align_windows_mates_rescue: NULL context%s", "");
	if (ctx_enter(c, cigar_pool, cigar_words)) return SSW_GPU_BUSY;
	return ctx_leave(c, align_windows_mates_rescue_locked(c, "align_windows_mates_rescue", Q, T, cand_off, nfrag, qidx, tidx, tbeg, tlen, nfwd, mate_q, prm,
	                                                      min_score, min_insert, max_insert, unpaired_penalty, orientation, 0, max_anchors, anchor_min_score,
	                                                      rescue_pad, sel, results, origin, cigar_pool, cigar_words));
}

/* ssw_gpu_align_windows_mates_rescue under a pair model: the rescue stage does not look at the table, the selection over the augmented list does */
int ssw_gpu_align_windows_mates_rescue_model(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int64_t* cand_off, int64_t nfrag,
                                             const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen, int32_t nfwd,
                                             const int32_t* mate_q, const ssw_gpu_params* prm, int32_t min_score, const ssw_gpu_pair_model* model,
                                             int32_t max_anchors, int32_t anchor_min_score, int32_t rescue_pad,
                                             ssw_gpu_mates* sel, ssw_gpu_result* results, ssw_gpu_rescued* origin, uint32_t** cigar_pool, int64_t* cigar_words)
{
	static const char who[] = "align_windows_mates_rescue_model";
	if (!c) return fail(0, "%s: NULL context", who);
	if (ctx_enter(c, cigar_pool, cigar_words)) return SSW_GPU_BUSY;
	if (!model) {      /* (the pool outputs are emptied as by every other refusal) */
		if (cigar_pool) *cigar_pool = 0;
		if (cigar_words) *cigar_words = 0;
		return ctx_leave(c, fail_who_d(c, who, "NULL argument", "model"));
	}
	return ctx_leave(c, align_windows_mates_rescue_locked(c, who, Q, T, cand_off, nfrag, qidx, tidx, tbeg, tlen, nfwd, mate_q, prm, min_score,
	                                                      model->min_insert, model->max_insert, model->unpaired_penalty, model->orientation,
	                                                      model->insert_penalty, max_anchors, anchor_min_score, rescue_pad, sel, results, origin,
	                                                      cigar_pool, cigar_words));
}

/* ------------------------------------------------------------------------------------------------
 * Best k candidate windows per read (ssw_gpu_align_windows_topk): the same select mode with k ranks per group (k_grouptopk).
 * Device state that outlives a fill launch, an input / output of the call like the window table: per candidate 48 bytes of record + 4 of
 * slot map (+ the 32 of the window table), per group 52 k + 4 bytes of output (k records of 48, k positions, one count) + 8 of offsets.
 * ------------------------------------------------------------------------------------------------ */
static int align_windows_topk_locked(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int64_t* cand_off, int64_t ng,
                                     const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen, const ssw_gpu_params* prm,
                                     int32_t k, int32_t min_score, int32_t max_drop, int32_t* pos, int32_t* n_eligible, ssw_gpu_result* results,
                                     uint32_t** cigar_pool, int64_t* cigar_words)
{
	char msg[200];
	if (cigar_pool) *cigar_pool = 0;      /* (as ssw_gpu_align_windows_best: the pool outputs are emptied before the argument checks) */
	if (cigar_words) *cigar_words = 0;
	if (k < 1 || k > SSW_GPU_GROUP_TOPK_MAX) {
		snprintf(msg, sizeof msg, "k = %d", k);
		return fail(c, "align_windows_topk: k must be 1 .. 64 (%s)", msg);
	}
	if (ng < 0 || (ng > 0 && (!cand_off || !pos || !n_eligible || !results))) return fail(c, "align_windows_topk: NULL argument%s", "");
	if (check_common(c, "align_windows_topk", Q, T, prm)) return -1;
	if (ng == 0) { memset(&c->tm, 0, sizeof c->tm); return 0; }
	if (ng > 0x7fffff00 / k) {
		snprintf(msg, sizeof msg, "%lld groups x %d", (long long)ng, k);
		return fail(c, "align_windows_topk: more than 2^31 output slots in one call (%s)", msg);
	}
	if (cand_off[0] != 0) {
		snprintf(msg, sizeof msg, "group 0 starts at candidate %lld", (long long)cand_off[0]);
		return fail(c, "align_windows_topk: cand_off[0] must be 0 (%s)", msg);
	}
	for (int64_t g = 0; g < ng; ++g)
		if (cand_off[g + 1] < cand_off[g]) {
			snprintf(msg, sizeof msg, "group %lld: candidates [%lld, %lld)", (long long)g, (long long)cand_off[g], (long long)cand_off[g + 1]);
			return fail(c, "align_windows_topk: cand_off decreases (%s)", msg);
		}
	const int64_t np = cand_off[ng];
	if (np > 0x7fffff00) return fail(c, "align_windows_topk: %s", "more than 2^31 candidates in one call");
	if (np > 0 && (!qidx || !tidx || !tbeg || !tlen)) return fail(c, "align_windows_topk: NULL argument%s", "");
	if (windows_check(c, "align_windows_topk", Q, T, qidx, tidx, tbeg, tlen, np)) return -1;
	if (np == 0) {      /* empty groups only */
		memset(&c->tm, 0, sizeof c->tm);
		for (int64_t o = 0; o < ng * k; ++o) { topk_pad(&results[o]); pos[o] = -1; }
		memset(n_eligible, 0, sizeof(int32_t) * (size_t)ng);
		return 0;
	}
	pair_src src; memset(&src, 0, sizeof src);
	src.tidx = tidx; src.tbeg = tbeg; src.tlen = tlen; src.who = "align_windows_topk";
	best_mode bm; memset(&bm, 0, sizeof bm);
	bm.cand_off = cand_off; bm.ngroups = ng; bm.min_score = min_score; bm.k = k; bm.max_drop = max_drop; bm.pos = pos; bm.n_eligible = n_eligible;
	return pairs_core(c, Q, T, qidx, &src, np, prm, results, cigar_pool, cigar_words, &bm);
}

int ssw_gpu_align_windows_topk(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const int64_t* cand_off, int64_t ngroups,
                               const int32_t* qidx, const int32_t* tidx, const int64_t* tbeg, const int32_t* tlen,
                               const ssw_gpu_params* prm, int32_t k, int32_t min_score, int32_t max_drop,
                               int32_t* pos, int32_t* n_eligible, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!c) return fail(0, "align_windows_topk: NULL context%s", "");
	if (ctx_enter(c, cigar_pool, cigar_words)) return SSW_GPU_BUSY;
	return ctx_leave(c, align_windows_topk_locked(c, Q, T, cand_off, ngroups, qidx, tidx, tbeg, tlen, prm, k, min_score, max_drop, pos, n_eligible,
	                                              results, cigar_pool, cigar_words));
}

/* ------------------------------------------------------------------------------------------------
 * Top-K database search (ssw_gpu_search_topk): the best k eligible targets of every query, selected on the device.
 *   streamed path (the fused database search's envelope): ssw_gpu_search_db's chunk loop in select mode -- k_topk merges every chunk's
 *   [nq][nt] compact records into per-query lists in HBM on the second stream, the lists come to the host once, at the end;
 *   generic path (SSW_NOT_STREAMABLE): full records per chunk, merged on the host with the same order -- exact, slower;
 *   flag != 0: the selected (query, target) pairs, in (q, r) order, through align_pairs_locked with the caller's parameters.
 * Queries go in blocks whose lists take at most half the budget; the two chunk buffers at most a quarter each.
 * ------------------------------------------------------------------------------------------------ */
static uint64_t topk_hkey(uint32_t score1, int32_t t) { return ((uint64_t)score1 << 32) | (uint32_t)~(uint32_t)t; }

typedef struct { uint64_t key; int32_t t; ssw_gpu_result r; } topk_cand;
static int topk_cand_cmp(const void* a, const void* b)
{
	const uint64_t x = ((const topk_cand*)a)->key, y = ((const topk_cand*)b)->key;
	return x < y ? 1 : x > y ? -1 : 0;      /* descending */
}

/* generic path of one query block: lists in lt[q * k ..] / lr[q * k ..], counts in cnt[] */
static int topk_generic(ssw_gpu_ctx* c, const ssw_gpu_seqs* V, const ssw_gpu_seqs* T, const ssw_gpu_params* p0, int32_t k, int32_t lo,
                        int64_t chunk, int32_t* lt, ssw_gpu_result* lr, call_acc* acc)
{
	const int32_t nq = V->count, nt_all = T->count;
	ssw_gpu_result* full = (ssw_gpu_result*)malloc(sizeof(ssw_gpu_result) * (size_t)nq * (size_t)chunk);
	topk_cand* cand = (topk_cand*)malloc(sizeof(topk_cand) * ((size_t)k + (size_t)chunk));
	int32_t* cnt = (int32_t*)calloc((size_t)nq, sizeof(int32_t));
	int rc = -1;
	if (!full || !cand || !cnt) { fail(c, "out of host memory (%s)", "top-K search"); goto out; }
	for (int32_t t0 = 0; t0 < nt_all; t0 += (int32_t)chunk) {
		const int32_t nt = nt_all - t0 < chunk ? nt_all - t0 : (int32_t)chunk;
		if (align_batch_locked(c, V, T, t0, nt, p0, full, 0, 0, 0)) goto out;
		timing_add(acc, &c->tm);
		for (int32_t q = 0; q < nq; ++q) {
			int32_t* qt = lt + (int64_t)q * k; ssw_gpu_result* qr = lr + (int64_t)q * k;
			const int32_t m0 = cnt[q];
			int32_t need = lo;
			if (m0 == k && (int32_t)qr[k - 1].score1 + 1 > need) need = qr[k - 1].score1 + 1;      /* ties stay with the lower target */
			int64_t n = 0;
			for (int32_t r = 0; r < m0; ++r) { cand[n].key = topk_hkey(qr[r].score1, qt[r]); cand[n].t = qt[r]; cand[n].r = qr[r]; ++n; }
			for (int32_t j = 0; j < nt; ++j) {
				const ssw_gpu_result* r = &full[(int64_t)q * nt + j];
				if (r->status != 0 || (int32_t)r->score1 < need) continue;
				cand[n].key = topk_hkey(r->score1, t0 + j); cand[n].t = t0 + j; cand[n].r = *r; ++n;
			}
			if (n == m0) continue;
			qsort(cand, (size_t)n, sizeof(topk_cand), topk_cand_cmp);
			const int32_t m = n < k ? (int32_t)n : k;
			for (int32_t r = 0; r < m; ++r) { qt[r] = cand[r].t; qr[r] = cand[r].r; }
			cnt[q] = m;
		}
	}
	rc = 0;
out:
	free(full); free(cand); free(cnt);
	return rc;
}

static int search_topk_locked(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const ssw_gpu_params* prm, int32_t k,
                              int32_t min_score, int32_t targets_per_chunk, int32_t* tidx, ssw_gpu_result* results,
                              uint32_t** cigar_pool, int64_t* cigar_words)
{
	const double t_start = wall_ms();
	const int32_t nq = Q->count, nt_all = T->count;
	if (cigar_pool) *cigar_pool = 0;
	if (cigar_words) *cigar_words = 0;
	memset(&c->tm, 0, sizeof c->tm);
	if (nq == 0) return 0;
	for (int64_t i = 0; i < (int64_t)nq * k; ++i) { tidx[i] = -1; topk_pad(&results[i]); }
	if (nt_all == 0) return 0;
	ssw_shim_set_device(c->device);
	if (ctx_side_streams(c)) return -1;
	/* the lists are decided by score1 alone, which the flag does not change: the search runs score-only, the caller's flag comes after */
	ssw_gpu_params p0 = *prm;
	if (p0.flag != 0) { p0.flag = 0; p0.mark_mismatch = 0; }
	const int32_t lo = min_score > 1 ? min_score : 1;
	int32_t cap = 64;
	while (cap < 2 * k) cap <<= 1;
	const int64_t per_q = (int64_t)k * (int64_t)(sizeof(int32_t) + sizeof(struct ssw_hit_rec)) + 2 * (int64_t)sizeof(int32_t);
	const int64_t budget = (int64_t)c->cm_budget;
	int64_t qb = budget / 2 / per_q;
	if (qb < 1) qb = 1;
	if (qb > nq) qb = nq;
	int64_t chunk = targets_per_chunk > 0 ? targets_per_chunk : 2048;
	const int64_t hits_lim = budget / 4 < ((int64_t)2 << 30) ? budget / 4 : ((int64_t)2 << 30);      /* bytes of one chunk buffer */
	while (chunk > 16 && qb * chunk * 16 > hits_lim) chunk /= 2;
	while (qb > 1 && qb * chunk * 16 > hits_lim) qb = (qb + 1) / 2;
	if (chunk > nt_all) chunk = nt_all;
	const int64_t nch = (nt_all + chunk - 1) / chunk;

	topk_sel sel; memset(&sel, 0, sizeof sel);
	call_acc acc; memset(&acc, 0, sizeof acc);
	int32_t* hlt = 0; struct ssw_hit_rec* hlh = 0; int32_t* hst = 0;
	int32_t *pq = 0, *pt = 0; int64_t* ppos = 0; ssw_gpu_result* pres = 0;
	int rc = -1;
	void* d_hits0 = ensure(c, &c->tk_hits0, (size_t)(qb * chunk * 16));
	void* d_hits1 = d_hits0 ? ensure(c, &c->tk_hits1, (size_t)(qb * chunk * 16)) : 0;
	unsigned char* d_lst = d_hits1 ? (unsigned char*)ensure(c, &c->tk_lst, (size_t)(qb * per_q + 64)) : 0;
	if (!d_lst) goto done;
	sel.ev = (void**)calloc((size_t)(2 * nch), sizeof(void*));
	hlt = (int32_t*)malloc(sizeof(int32_t) * (size_t)(qb * k));
	hlh = (struct ssw_hit_rec*)malloc(sizeof(struct ssw_hit_rec) * (size_t)(qb * k));
	hst = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)qb);
	if (!sel.ev || !hlt || !hlh || !hst) { fail(c, "out of host memory (%s)", "top-K search"); goto done; }
	for (int64_t i = 0; i < 2 * nch; ++i) { sel.ev[i] = ssw_shim_event_create(); if (!sel.ev[i]) { fail(c, "event creation failed: %s", ssw_shim_last_error()); goto done; } sel.nev = (int)(i + 1); }
	/* list layout: states [qb][2], targets [qb][k], records [qb][k] (16-byte aligned) */
	int32_t* d_state = (int32_t*)d_lst;
	int32_t* d_lt = d_state + 2 * qb;
	struct ssw_hit_rec* d_lh = (struct ssw_hit_rec*)(d_lst + ((size_t)(2 * qb + qb * k) * sizeof(int32_t) + 15) / 16 * 16);

	for (int64_t q0 = 0; q0 < nq; q0 += qb) {
		const int32_t nb = (int32_t)(nq - q0 < qb ? nq - q0 : qb);
		struct ssw_gpu_seqs V; V.ctx = c; V.d_codes = Q->d_codes; V.d_off = Q->d_off + q0; V.h_off = Q->h_off + q0; V.count = nb;
		V.total = V.h_off[nb] - V.h_off[0];
		int32_t* lt = tidx + q0 * k; ssw_gpu_result* lr = results + q0 * k;
		if (ssw_shim_memset(d_state, 0, sizeof(int32_t) * 2 * (size_t)nb, c->stream)) { fail(c, "memset failed: %s", ssw_shim_last_error()); goto done; }
		sel.a.hits = 0; sel.a.nq = nb; sel.a.nt = 0; sel.a.tfirst = 0; sel.a.k = k; sel.a.cap = cap; sel.a.min_score = lo;
		sel.a.lst_t = d_lt; sel.a.lst_h = d_lh; sel.a.state = d_state;
		db_stream ds; memset(&ds, 0, sizeof ds);
		ds.chunk = (int32_t)chunk; ds.sel = &sel;
		ds.d_hits[0] = (struct ssw_hit_rec*)d_hits0; ds.d_hits[1] = (struct ssw_hit_rec*)d_hits1;
		const int brc = align_batch_locked(c, &V, T, 0, nt_all, &p0, 0, 0, 0, &ds);
		if (brc == SSW_NOT_STREAMABLE) {
			ssw_shim_stream_sync(c->stream); ssw_shim_stream_sync(c->stream2);
			if (topk_generic(c, &V, T, &p0, k, lo, chunk, lt, lr, &acc)) goto done;
			continue;
		}
		if (brc) { ssw_shim_stream_sync(c->stream); ssw_shim_stream_sync(c->stream2); goto done; }
		double sel_ms = 0;
		for (int64_t i = 0; i < nch; ++i) sel_ms += ssw_shim_event_elapsed_ms(sel.ev[2 * i], sel.ev[2 * i + 1]);
		c->tm.reduce_ms = sel_ms;      /* (include/ssw_gpu.h: the selection's device time) */
		timing_add(&acc, &c->tm);
		/* the lists, once */
		if (ssw_shim_d2h(hst, d_state, sizeof(int32_t) * 2 * (size_t)nb, c->stream) ||
		    ssw_shim_d2h(hlt, d_lt, sizeof(int32_t) * (size_t)nb * (size_t)k, c->stream) ||
		    ssw_shim_d2h(hlh, d_lh, sizeof(struct ssw_hit_rec) * (size_t)nb * (size_t)k, c->stream) || ssw_shim_stream_sync(c->stream)) {
			fail(c, "result download failed: %s", ssw_shim_last_error()); goto done;
		}
		for (int32_t q = 0; q < nb; ++q) {
			const int32_t m = hst[2 * q];
			if (m < 0 || m > k) { fail(c, "top-K search: %s", "corrupt list state"); goto done; }
			for (int32_t r = 0; r < m; ++r) {      /* a score-only record is what the hit record says (k_filldb writes both from the same values) */
				const struct ssw_hit_rec* h = &hlh[(int64_t)q * k + r];
				ssw_gpu_result* o = &lr[(int64_t)q * k + r];
				lt[(int64_t)q * k + r] = hlt[(int64_t)q * k + r];
				o->score1 = h->score1; o->score2 = h->score2; o->ref_end1 = h->ref_end1; o->read_end1 = h->read_end1; o->ref_end2 = h->ref_end2;
			}
		}
	}
	if (prm->flag != 0) {      /* begins, CIGARs, mark_mismatch: the selected pairs through the pair path, with the caller's parameters */
		int64_t np = 0;
		for (int64_t i = 0; i < (int64_t)nq * k; ++i) np += tidx[i] >= 0;
		pq = (int32_t*)malloc(sizeof(int32_t) * (size_t)(np > 0 ? np : 1)); pt = (int32_t*)malloc(sizeof(int32_t) * (size_t)(np > 0 ? np : 1));
		ppos = (int64_t*)malloc(sizeof(int64_t) * (size_t)(np > 0 ? np : 1)); pres = (ssw_gpu_result*)malloc(sizeof(ssw_gpu_result) * (size_t)(np > 0 ? np : 1));
		if (!pq || !pt || !ppos || !pres) { fail(c, "out of host memory (%s)", "top-K pairs"); goto done; }
		int64_t p = 0;
		for (int64_t i = 0; i < (int64_t)nq * k; ++i) if (tidx[i] >= 0) { pq[p] = (int32_t)(i / k); pt[p] = tidx[i]; ppos[p] = i; ++p; }
		if (align_pairs_locked(c, Q, T, pq, pt, np, prm, pres, cigar_pool, cigar_words)) goto done;
		timing_add(&acc, &c->tm);
		for (int64_t i = 0; i < np; ++i) results[ppos[i]] = pres[i];
	}
	acc.t.total_ms = wall_ms() - t_start;
	c->tm = acc.t;
	rc = 0;
done:
	for (int i = 0; i < sel.nev; ++i) ssw_shim_event_destroy(sel.ev[i]);
	free(sel.ev); free(hlt); free(hlh); free(hst); free(pq); free(pt); free(ppos); free(pres);
	return rc;
}

int ssw_gpu_search_topk(ssw_gpu_ctx* c, const ssw_gpu_seqs* Q, const ssw_gpu_seqs* T, const ssw_gpu_params* prm, int32_t k, int32_t min_score,
                        int32_t targets_per_chunk, int32_t* tidx, ssw_gpu_result* results, uint32_t** cigar_pool, int64_t* cigar_words)
{
	if (!c) return fail(0, "search_topk: NULL context%s", "");
	if (k < 1 || k > SSW_GPU_TOPK_MAX) return fail(c, "search_topk: k must be 1 .. SSW_GPU_TOPK_MAX%s", "");
	if (!tidx || !results) return fail(c, "search_topk: NULL argument%s", "");
	if (check_common(c, "search_topk", Q, T, prm)) return -1;      /* (this entry point checks its arguments before it takes the context) */
	if (ctx_enter(c, cigar_pool, cigar_words)) return SSW_GPU_BUSY;
	return ctx_leave(c, search_topk_locked(c, Q, T, prm, k, min_score, targets_per_chunk, tidx, results, cigar_pool, cigar_words));
}

void* ssw_gpu_host_alloc(ssw_gpu_ctx* c, size_t bytes)
{
	if (!c) return 0;
	ssw_shim_set_device(c->device);
	void* p = ssw_shim_host_alloc(bytes);
	if (!p) fail(c, "page-locked host allocation failed: %s", ssw_shim_last_error());
	return p;
}

void ssw_gpu_host_free(ssw_gpu_ctx* c, void* p)
{
	if (!c || !p) return;
	ssw_shim_set_device(c->device);
	ssw_shim_host_free(p);
}

#ifdef SSW_GPU_TEST_HOOKS      /* diagnostics: libssw_hooks.so and the emulator only (include/ssw_gpu_diag.h) */
int ssw_gpu_selftest_lanes(ssw_gpu_ctx* c, uint32_t* out1024)
{
	if (!c || !out1024) return -1;
	ssw_shim_set_device(c->device);
	uint32_t* d = (uint32_t*)ssw_shim_malloc(1024 * 4);
	if (!d) return fail(c, "device allocation failed: %s", ssw_shim_last_error());
	ssw_selftest_args a; a.lanes_out = d; a.sink = 0; a.iters = 0; a.seed = 0;
	int rc = ssw_shim_launch_selftest(&a, 1, c->stream) || ssw_shim_d2h(out1024, d, 1024 * 4, c->stream) || ssw_shim_stream_sync(c->stream);
	ssw_shim_free(d);
	return rc ? fail(c, "selftest failed: %s", ssw_shim_last_error()) : 0;
}

/* measured packed-int16 VALU rate of the device in lane-operations per second (both 16-bit halves count as one) */
double ssw_gpu_valu_probe(ssw_gpu_ctx* c, int32_t blocks, int32_t iters)
{
	if (!c || blocks < 1 || iters < 1) return -1.0;
	ssw_shim_set_device(c->device);
	uint32_t* sink = (uint32_t*)ssw_shim_malloc((size_t)blocks * 256 * 4);
	if (!sink) return -1.0;
	ssw_selftest_args a; a.lanes_out = 0; a.sink = sink; a.iters = iters; a.seed = 0x00030001u;
	double best = -1.0;
	for (int rep = 0; rep < 3; ++rep) {
		ssw_shim_event_record(c->ev_a, c->stream);
		if (ssw_shim_launch_selftest(&a, blocks, c->stream)) break;
		ssw_shim_event_record(c->ev_b, c->stream);
		if (ssw_shim_stream_sync(c->stream)) break;
		double ms = ssw_shim_event_elapsed_ms(c->ev_a, c->ev_b);
		double rate = (double)blocks * 256.0 * iters * 96.0 / (ms * 1e-3);
		if (rate > best) best = rate;
	}
	ssw_shim_free(sink);
	return best;
}
#endif

s_align* ssw_gpu_result_to_align(const ssw_gpu_result* r, const uint32_t* cigar_pool)
{
	if (!r || r->status != 0) return 0;
	s_align* a = (s_align*)calloc(1, sizeof(s_align));
	a->score1 = r->score1; a->score2 = r->score2; a->ref_begin1 = r->ref_begin1; a->ref_end1 = r->ref_end1;
	a->read_begin1 = r->read_begin1; a->read_end1 = r->read_end1; a->ref_end2 = r->ref_end2; a->flag = r->flag;
	if (r->cigarLen > 0 && cigar_pool && r->cigar_off >= 0) {
		a->cigar = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)r->cigarLen);
		memcpy(a->cigar, cigar_pool + r->cigar_off, sizeof(uint32_t) * (size_t)r->cigarLen);
		a->cigarLen = r->cigarLen;
	}
	return a;
}

/* ------------------------------------------------------------------------------------------------
 * ssw.h single-pair ABI on top of the batch path.
 *
 * The reference is re-entrant: no mutable global state, concurrent ssw_align on one const s_profile* is legal
 * (src/ssw.c:855-977).  Here every calling thread gets its own implicit context on first use -- devices are handed out
 * round-robin (SSW_GPU_DEVICE pins all of them to one) -- so calls from different threads never share streams or
 * workspaces and run concurrently.  Per thread the context keeps pooled device buffers for the query and the target
 * (no hipMalloc / hipFree per call) and remembers the last target: callers loop "for each read: for each target"
 * (src/main.c:462-526) and hand in the same reference over and over; it is re-uploaded only when its bytes changed
 * (compared against a host copy -- the caller may reuse one buffer for different targets, as main.c does).
 * ------------------------------------------------------------------------------------------------ */
typedef struct implicit_ctx_s {
	struct implicit_ctx_s* next;    /* parked contexts (below) */
	ssw_gpu_ctx* ctx;
	ssw_gpu_seqs q, t;              /* one-sequence sets over pooled device buffers */
	int64_t q_hoff[2], t_hoff[2];
	size_t qcap, tcap;              /* device code capacity */
	int8_t* tcopy; size_t tcopy_cap; int t_valid;     /* bytes of the target that is resident in t */
	unsigned char* stage; size_t stage_cap;           /* host staging of one upload (offsets + codes) */
} implicit_ctx;

static int g_single_inflight;      /* ssw_align calls of this process inside the library right now */
static pthread_key_t g_ictx_key;
static pthread_once_t g_ictx_once = PTHREAD_ONCE_INIT;
static int g_next_device = 0;

/* A caller thread that ends PARKS its context; the next new caller thread takes it over (streams, events and pooled buffers are process-wide
   objects: nothing in them belongs to the thread that created them).  The thread-exit hook must not call into the HIP runtime: it runs as a
   pthread-key destructor, i.e. AFTER the C++ thread_local objects of the exiting thread -- the runtime's own per-thread state among them --
   have been destroyed, and a hipFree / hipStreamDestroy from there works on freed memory.  Round 4's hook closed the context right there;
   with 16 caller threads ending together that corrupted the heap now and then (a crash at process exit, found with the round-5 latency
   harness).  Parked contexts are reused by the next new caller thread; more than SSW_PARK_MAX of them are closed by the next LIVE thread that
   comes through implicit_get (new or not), and ssw_gpu_release_parked() closes all of them (round-5 advisor: after a burst of N caller threads the process
   kept N contexts' HBM until exit).  What is still parked at process exit goes with the process. */
#define SSW_PARK_MAX 4
static pthread_mutex_t g_park_mu = PTHREAD_MUTEX_INITIALIZER;
static implicit_ctx* g_parked;
static int g_nparked;
static void implicit_destroy(void* p)
{
	implicit_ctx* ic = (implicit_ctx*)p;
	if (!ic) return;
	pthread_mutex_lock(&g_park_mu);
	ic->next = g_parked; g_parked = ic; ++g_nparked;
	pthread_mutex_unlock(&g_park_mu);
}
static void implicit_free(implicit_ctx* ic)      /* from a live thread only (HIP calls inside) */
{
	ssw_gpu_ctx* c = ic->ctx;
	ssw_shim_set_device(c->device);
	ssw_shim_stream_sync(c->stream);
	if (ic->q.d_off) ssw_shim_free(ic->q.d_off);
	if (ic->t.d_off) ssw_shim_free(ic->t.d_off);
	free(ic->tcopy); free(ic->stage);
	ssw_gpu_close(c);
	free(ic);
}
/* closes the parked contexts beyond `keep`; returns how many were closed */
static int parked_trim(int keep)
{
	implicit_ctx* drop = 0; int n = 0;
	pthread_mutex_lock(&g_park_mu);
	while (g_nparked > keep && g_parked) { implicit_ctx* ic = g_parked; g_parked = ic->next; --g_nparked; ic->next = drop; drop = ic; }
	pthread_mutex_unlock(&g_park_mu);
	while (drop) { implicit_ctx* ic = drop; drop = ic->next; implicit_free(ic); ++n; }
	return n;
}
int ssw_gpu_release_parked(void) { return parked_trim(0); }
/* Runs once per process, before the first implicit context exists (pthread_once), not from every first-calling thread.
   Caller threads' calls overlap on the device only as far as the runtime has hardware queues for their streams: ROCm's default is four
   per process; eight made 8 caller threads 6 085 -> 8 146 calls per second (profiles/round4_dropin_threads.txt).  Rounds 4-5 asked for
   eight by themselves (setenv GPU_MAX_HW_QUEUES); a drop-in library does not change process-wide runtime configuration unasked (round-5
   verdict): it is OPT-IN now -- SSW_GPU_HW_QUEUES=<n> in the environment makes the library ask for n queues if nobody set
   GPU_MAX_HW_QUEUES and the runtime is not up yet; without it the environment is left alone. */
static void implicit_key_init(void)
{
	pthread_key_create(&g_ictx_key, implicit_destroy);
	const char* q = getenv("SSW_GPU_HW_QUEUES");
	if (q && q[0] >= '1' && q[0] <= '9') setenv("GPU_MAX_HW_QUEUES", q, 0);
}

static implicit_ctx* implicit_get(void)
{
	pthread_once(&g_ictx_once, implicit_key_init);
	implicit_ctx* ic = (implicit_ctx*)pthread_getspecific(g_ictx_key);
	if (ic) {      /* (any live caller applies the cap, not only a new thread: a burst of short-lived threads may park its contexts after the last new thread came by) */
		if (__atomic_load_n(&g_nparked, __ATOMIC_RELAXED) > SSW_PARK_MAX) parked_trim(SSW_PARK_MAX);
		return ic;
	}
	pthread_mutex_lock(&g_park_mu);      /* a context parked by a caller thread that ended: taken over as it is (its device, its buffers, its resident target) */
	ic = g_parked;
	if (ic) { g_parked = ic->next; --g_nparked; }
	pthread_mutex_unlock(&g_park_mu);
	parked_trim(SSW_PARK_MAX);            /* (this thread is alive: it may call into the runtime) */
	if (ic) { ic->next = 0; pthread_setspecific(g_ictx_key, ic); return ic; }
	const int ndev = ssw_shim_device_count();
	const char* e = getenv("SSW_GPU_DEVICE");
	const int dev = e ? atoi(e) : (ndev > 0 ? __atomic_fetch_add(&g_next_device, 1, __ATOMIC_RELAXED) % ndev : 0);
	ssw_gpu_ctx* c = ssw_gpu_open(dev);
	if (!c) return 0;
	ic = (implicit_ctx*)calloc(1, sizeof *ic);
	if (!ic) { ssw_gpu_close(c); fail(0, "out of host memory%s", ""); return 0; }
	ic->ctx = c;
	ic->q.ctx = c; ic->q.count = 1; ic->q.h_off = ic->q_hoff;
	ic->t.ctx = c; ic->t.count = 1; ic->t.h_off = ic->t_hoff;
	pthread_setspecific(g_ictx_key, ic);
	return ic;
}

/* (re)fill a pooled one-sequence set; the copies are ordered before the kernels of the batch call on the same stream */
static int implicit_load(implicit_ctx* ic, ssw_gpu_seqs* s, size_t* cap, const int8_t* codes, int32_t len)
{
	/* offsets and codes live in ONE device allocation -- [0, len as int64][codes] -- and travel in one copy from a staging buffer: a
	   single-pair call is bound by the number of dependent operations on its stream */
	ssw_gpu_ctx* c = ic->ctx;
	if (!s->d_off || *cap < (size_t)len + 64) {
		if (s->d_off) { ssw_shim_stream_sync(c->stream); ssw_shim_free(s->d_off); s->d_off = 0; s->d_codes = 0; *cap = 0; }
		const size_t want = (size_t)len + (size_t)len / 4 + 4096;
		s->d_off = (int64_t*)ssw_shim_malloc(want + 16);
		if (!s->d_off) return fail(c, "device allocation failed: %s", ssw_shim_last_error());
		s->d_codes = (int8_t*)s->d_off + 16;
		*cap = want;
	}
	if (ic->stage_cap < (size_t)len + 16) {
		free(ic->stage);
		ic->stage_cap = (size_t)len + (size_t)len / 4 + 4096;
		ic->stage = (unsigned char*)malloc(ic->stage_cap);
		if (!ic->stage) { ic->stage_cap = 0; return fail(c, "out of host memory%s", ""); }
	}
	s->h_off[0] = 0; s->h_off[1] = len; s->total = len;
	memcpy(ic->stage, s->h_off, 16);
	if (len > 0) memcpy(ic->stage + 16, codes, (size_t)len);
	if (ssw_shim_h2d(s->d_off, ic->stage, (size_t)len + 16, c->stream)) return fail(c, "upload failed: %s", ssw_shim_last_error());
	return 0;
}

s_profile* ssw_init(const int8_t* read, const int32_t readLen, const int8_t* mat, const int32_t n, const int8_t score_size)
{
	/* the reference has no error return here and reads `readLen` residues unconditionally; a negative length or missing
	   arrays can only be a caller bug, so they are refused (ssw_align then reports the missing profile) */
	if (readLen < 0 || (readLen > 0 && !read) || !mat || n < 1) {
		fprintf(stderr, "ssw_init: invalid arguments (readLen %d, n %d).\n", (int)readLen, (int)n);
		return 0;
	}
	s_profile* p = (s_profile*)calloc(1, sizeof(struct _profile));
	if (!p) return 0;
	p->read = read; p->mat = mat; p->readLen = readLen; p->n = n; p->score_size = score_size;
	return p;
}

void init_destroy(s_profile* p) { free(p); }

void align_destroy(s_align* a) { if (a) { free(a->cigar); free(a); } }

s_align* ssw_align(const s_profile* prof, const int8_t* ref, int32_t refLen, const uint8_t weight_gapO,
                   const uint8_t weight_gapE, const uint8_t flag, const uint16_t filters, const int32_t filterd,
                   const int32_t maskLen)
{
	s_align* out = 0;
	if (!prof || prof->score_size < 0 || prof->score_size > 2) {
		fprintf(stderr, "Please call the function ssw_init before ssw_align.\n");
		return 0;
	}
	if (maskLen < 15)
		fprintf(stderr, "When maskLen < 15, the function ssw_align doesn't return 2nd best alignment information.\n");
	if (refLen < 0 || (refLen > 0 && !ref)) { fprintf(stderr, "ssw_align: invalid reference (refLen %d).\n", (int)refLen); return 0; }
	implicit_ctx* ic = implicit_get();
	if (!ic) {
		fprintf(stderr, "ssw_align: %s\n", ssw_gpu_last_error(0));
		return 0;
	}
	ssw_gpu_ctx* c = ic->ctx;
	CALL_TRACE("ssw_align: enter");
	ssw_shim_set_device(c->device);
	int ok = 1;
	if (ok && !(ic->t_valid && ic->t.total == refLen && (refLen == 0 || memcmp(ic->tcopy, ref, (size_t)refLen) == 0))) {
		ic->t_valid = 0;
		if (ic->tcopy_cap < (size_t)refLen) {
			free(ic->tcopy);
			ic->tcopy = (int8_t*)malloc((size_t)refLen + (size_t)refLen / 4 + 64);
			ic->tcopy_cap = ic->tcopy ? (size_t)refLen + (size_t)refLen / 4 + 64 : 0;
		}
		ok = implicit_load(ic, &ic->t, &ic->tcap, ref, refLen) == 0;
		if (ok) ok = ssw_shim_stream_sync(c->stream) == 0;      /* (the staging buffer is about to be reused for the query) */
		if (ok && ic->tcopy) { memcpy(ic->tcopy, ref, (size_t)refLen); ic->t_valid = 1; }   /* no host copy: the target is simply uploaded every time */
	}
	if (ok) ok = implicit_load(ic, &ic->q, &ic->qcap, prof->read, prof->readLen) == 0;
	if (ok) {
		ssw_gpu_params prm;
		prm.mat = prof->mat; prm.n = prof->n; prm.gapO = weight_gapO; prm.gapE = weight_gapE; prm.flag = flag;
		prm.filters = filters; prm.filterd = filterd; prm.maskLen = maskLen < 0 ? 0 : maskLen; prm.score_size = prof->score_size; prm.mark_mismatch = 0;
		ssw_gpu_result r; uint32_t* pool = 0; int64_t words = 0;
		/* how many caller threads are in here at once: alone, a call spreads its one pair over the whole device (tiles of half a halo,
		   lowest latency); with company it takes its share, fewer and longer tiles with less recomputed halo */
		c->device_share = __atomic_add_fetch(&g_single_inflight, 1, __ATOMIC_RELAXED);
		const int brc = ssw_gpu_align_batch(c, &ic->q, &ic->t, 0, 1, &prm, &r, &pool, &words);
		__atomic_sub_fetch(&g_single_inflight, 1, __ATOMIC_RELAXED);
		c->device_share = 0;
		if (brc == 0) {
			if (r.status == 1)
				fprintf(stderr, "Please set 2 to the score_size parameter of the function ssw_init, otherwise the alignment results will be incorrect.\n");
			else {
				out = ssw_gpu_result_to_align(&r, pool);
				if (out && out->flag == 2)
					fprintf(stderr, "Warning: The alignment path of one pair of sequences may miss a small part. [ssw.c ssw_align]\n");
			}
		} else { fprintf(stderr, "ssw_align: %s\n", ssw_gpu_last_error(c)); ic->t_valid = 0; }
		free(pool);
	} else { fprintf(stderr, "ssw_align: %s\n", ssw_gpu_last_error(c)); ic->t_valid = 0; }
	CALL_TRACE("ssw_align: return");
	return out;
}
