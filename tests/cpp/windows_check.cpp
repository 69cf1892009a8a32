// tests/cpp/windows_check.cpp -- TEST INFRASTRUCTURE.  BatchAligner::AlignWindows (include/ssw_gpu_cpp.h) over windows of a few resident
// references against BatchAligner::AlignPairs of a second aligner whose references ARE those windows, cut out on the host: every field of
// every Alignment, cigar vector and string, and the flag must be equal; with rebase = true the three reference positions move by the
// window's begin.  Usage: windows_check [pairs] [references]   -> prints "ok <pairs>" or the first differences; exit code 0 / 1.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "ssw_gpu_cpp.h"

static unsigned long long rng_state = 0xD1B54A32D192ED03ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 11); }

typedef StripedSmithWaterman::Alignment Aln;

static bool same(const Aln& e, const Aln& g, int shift)
{
	return e.sw_score == g.sw_score && e.sw_score_next_best == g.sw_score_next_best && e.ref_begin + (e.ref_begin >= 0 ? shift : 0) == g.ref_begin &&
	       e.ref_end + (e.ref_end >= 0 ? shift : 0) == g.ref_end && e.query_begin == g.query_begin && e.query_end == g.query_end &&
	       e.ref_end_next_best + (e.ref_end_next_best >= 0 ? shift : 0) == g.ref_end_next_best && e.mismatches == g.mismatches &&
	       e.cigar_string == g.cigar_string && e.cigar == g.cigar;
}

int main(int argc, char** argv)
{
	const int np = argc > 1 ? atoi(argv[1]) : 24, nr = argc > 2 ? atoi(argv[2]) : 4;
	const char acgt[] = "ACGT";
	std::vector<std::string> refs;
	for (int t = 0; t < nr; ++t) {
		std::string s;
		const int L = 300 + (int)(rnd() % 500) + t;
		for (int i = 0; i < L; ++i) s += acgt[rnd() % 4];
		refs.push_back(s);
	}
	std::vector<std::string> queries, cut;
	std::vector<StripedSmithWaterman::BatchAligner::Window> windows;
	std::vector<int32_t> cut_index;
	for (int i = 0; i < np; ++i) {
		StripedSmithWaterman::BatchAligner::Window w;
		w.reference = (int32_t)(rnd() % (unsigned)nr);
		const std::string& ref = refs[(size_t)w.reference];
		w.length = 60 + (int32_t)(rnd() % 200);
		if (i == 0) { w.begin = 0; w.length = (int32_t)ref.size(); }                                   // the whole reference
		else if (i == 1) w.begin = (int64_t)ref.size() - w.length;                                     // ends on the last residue
		else w.begin = (int64_t)(rnd() % (unsigned)(ref.size() - (size_t)w.length + 1));
		const std::string win = ref.substr((size_t)w.begin, (size_t)w.length);
		const int L = 20 + (int)(rnd() % 40), p = (int)(rnd() % (unsigned)(win.size() - (size_t)L + 1));
		std::string q = win.substr((size_t)p, (size_t)L);
		for (size_t k = 0; k < q.size(); ++k) if (rnd() % 20 == 0) q[k] = acgt[rnd() % 4];
		if (i % 7 == 3) q.erase(q.size() / 2, 2);                                                      // a deletion in the read
		queries.push_back(q); windows.push_back(w); cut.push_back(win); cut_index.push_back(i);
	}
	StripedSmithWaterman::BatchAligner al(2, 2, 3, 1), al_cut(2, 2, 3, 1);
	al.SetReferenceSequences(refs);
	al_cut.SetReferenceSequences(cut);
	int bad = 0;
	for (int mode = 0; mode < 2; ++mode) {
		StripedSmithWaterman::Filter filter;
		if (mode == 1) { filter.report_cigar = false; filter.report_begin_position = false; }
		std::vector<Aln> got, got_rebased, exp;
		std::vector<uint16_t> gflags, eflags;
		al.AlignWindows(queries, windows, filter, &got, 20, false, &gflags);
		al.AlignWindows(queries, windows, filter, &got_rebased, 20, true);
		al_cut.AlignPairs(queries, cut_index, filter, &exp, 20, &eflags);
		for (int i = 0; i < np; ++i) {
			const bool ok = same(exp[(size_t)i], got[(size_t)i], 0) && gflags[(size_t)i] == eflags[(size_t)i] &&
			                same(exp[(size_t)i], got_rebased[(size_t)i], (int)windows[(size_t)i].begin);
			if (!ok && ++bad <= 5)
				printf("mode %d pair %d (reference %d, begin %lld, length %d): expected score %u [%d, %d] '%s', got score %u [%d, %d] '%s', rebased [%d, %d]\n", mode, i,
				       windows[(size_t)i].reference, (long long)windows[(size_t)i].begin, windows[(size_t)i].length, exp[(size_t)i].sw_score, exp[(size_t)i].ref_begin,
				       exp[(size_t)i].ref_end, exp[(size_t)i].cigar_string.c_str(), got[(size_t)i].sw_score, got[(size_t)i].ref_begin, got[(size_t)i].ref_end,
				       got[(size_t)i].cigar_string.c_str(), got_rebased[(size_t)i].ref_begin, got_rebased[(size_t)i].ref_end);
		}
	}
	bool threw = false;      // a window that leaves its reference is refused, not clamped
	try {
		std::vector<StripedSmithWaterman::BatchAligner::Window> w1(1, windows[0]);
		w1[0].begin = 1;
		std::vector<std::string> q1(1, queries[0]);
		std::vector<Aln> out;
		al.AlignWindows(q1, w1, StripedSmithWaterman::Filter(), &out, 20);
	} catch (const std::runtime_error&) { threw = true; }
	if (!threw) { printf("a window beyond its reference's end was accepted\n"); ++bad; }
	if (bad) { printf("%d differences\n", bad); return 1; }
	printf("ok %d\n", np);
	return 0;
}
