/* Native baseline of scripts/gpu_pairs_bench.py: the mapper's loop "for each pair: ssw_init + ssw_align" over a pair list on T threads,
   against whichever libssw.so-compatible library is named (this library, or the reference built into oracle/_ref).
   usage: pairs_loop <lib.so> <pairs.bin> <threads> <flag>    pairs.bin (little endian):
     int32 n, int32 gapO, int32 gapE, int32 npairs, int8 mat[n*n], then per pair: int32 qlen, int32 tlen, qlen + tlen int8 codes
   prints "<seconds> <cells>" */
#include <dlfcn.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

typedef void* (*init_fn)(const int8_t*, int32_t, const int8_t*, int32_t, int8_t);
typedef void (*initd_fn)(void*);
typedef void* (*align_fn)(const void*, const int8_t*, int32_t, uint8_t, uint8_t, uint8_t, uint16_t, int32_t, int32_t);
typedef void (*alignd_fn)(void*);
static init_fn f_init; static initd_fn f_initd; static align_fn f_align; static alignd_fn f_alignd;
static int32_t n, gapO, gapE, npairs, flag, nthreads;
static int8_t* mat; static int32_t* ql; static int32_t* tl; static int8_t** qp; static int8_t** tp;

static void* work(void* arg)
{
	const int64_t t = (int64_t)(intptr_t)arg;
	for (int64_t i = t; i < npairs; i += nthreads) {
		void* p = f_init(qp[i], ql[i], mat, n, 2);
		void* a = f_align(p, tp[i], tl[i], (uint8_t)gapO, (uint8_t)gapE, (uint8_t)flag, 0, 0, ql[i] / 2);
		if (a) f_alignd(a);
		f_initd(p);
	}
	return 0;
}

int main(int argc, char** argv)
{
	if (argc < 5) { fprintf(stderr, "usage: pairs_loop lib.so pairs.bin threads flag\n"); return 2; }
	void* L = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
	if (!L) { fprintf(stderr, "%s\n", dlerror()); return 1; }
	f_init = (init_fn)dlsym(L, "ssw_init"); f_initd = (initd_fn)dlsym(L, "init_destroy");
	f_align = (align_fn)dlsym(L, "ssw_align"); f_alignd = (alignd_fn)dlsym(L, "align_destroy");
	FILE* f = fopen(argv[2], "rb");
	if (!f || !f_init || !f_initd || !f_align || !f_alignd) { fprintf(stderr, "cannot open input or resolve symbols\n"); return 1; }
	nthreads = atoi(argv[3]); flag = atoi(argv[4]);
	int32_t h[4];
	if (fread(h, 4, 4, f) != 4) return 1;
	n = h[0]; gapO = h[1]; gapE = h[2]; npairs = h[3];
	mat = malloc((size_t)n * n); ql = malloc(4 * (size_t)npairs); tl = malloc(4 * (size_t)npairs);
	qp = malloc(sizeof(int8_t*) * (size_t)npairs); tp = malloc(sizeof(int8_t*) * (size_t)npairs);
	if (fread(mat, 1, (size_t)n * n, f) != (size_t)n * n) return 1;
	double cells = 0;
	for (int32_t i = 0; i < npairs; ++i) {
		int32_t l[2];
		if (fread(l, 4, 2, f) != 2) return 1;
		ql[i] = l[0]; tl[i] = l[1];
		qp[i] = malloc((size_t)l[0] + 1); tp[i] = malloc((size_t)l[1] + 1);
		if (fread(qp[i], 1, (size_t)l[0], f) != (size_t)l[0] || fread(tp[i], 1, (size_t)l[1], f) != (size_t)l[1]) return 1;
		cells += (double)l[0] * l[1];
	}
	fclose(f);
	pthread_t* th = malloc(sizeof(pthread_t) * (size_t)nthreads);
	struct timespec a, b;
	clock_gettime(CLOCK_MONOTONIC, &a);
	for (int t = 0; t < nthreads; ++t) pthread_create(&th[t], 0, work, (void*)(intptr_t)t);
	for (int t = 0; t < nthreads; ++t) pthread_join(th[t], 0);
	clock_gettime(CLOCK_MONOTONIC, &b);
	printf("%.6f %.0f\n", (b.tv_sec - a.tv_sec) + (b.tv_nsec - a.tv_nsec) * 1e-9, cells);
	return 0;
}
