// tests/cpp/topk_check.cpp -- TEST INFRASTRUCTURE.  BatchAligner::SearchTopK (include/ssw_gpu_cpp.h) against BatchAligner::AlignPairs over
// every (query, reference) pair of the same seeded set: the ranks are derived from the pair scores (sw_score descending, reference index
// ascending, scores > 0 and >= min_score), and every hit's Alignment -- every field, cigar vector and string -- and flag must equal the pair's.
// Usage: topk_check [queries] [references] [k] [min_score]   -> prints "ok <hits>" or the first differences; exit code 0 / 1.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>

#include "ssw_gpu_cpp.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 11); }

int main(int argc, char** argv)
{
	const int nq = argc > 1 ? atoi(argv[1]) : 8, nr = argc > 2 ? atoi(argv[2]) : 40, k = argc > 3 ? atoi(argv[3]) : 5;
	const int min_score = argc > 4 ? atoi(argv[4]) : 1;
	const char acgt[] = "ACGT";
	std::vector<std::string> refs;
	for (int t = 0; t < nr; ++t) {
		std::string s;
		const int L = 40 + (int)(rnd() % 160);
		for (int i = 0; i < L; ++i) s += acgt[rnd() % 4];
		refs.push_back(s);
	}
	for (int t = 5; t < nr; t += 7) refs[(size_t)t] = refs[(size_t)(t - 5)];      // duplicates: equal scores, ranked by index
	std::vector<std::string> queries;
	for (int q = 0; q < nq; ++q) {
		const std::string& src = refs[rnd() % (unsigned)nr];
		const int L = 20 + (int)(rnd() % 30), p = (int)(rnd() % (unsigned)(src.size() - L));
		std::string s = src.substr((size_t)p, (size_t)L);
		for (size_t i = 0; i < s.size(); ++i) if (rnd() % 25 == 0) s[i] = acgt[rnd() % 4];
		queries.push_back(s);
	}
	StripedSmithWaterman::BatchAligner al(2, 2, 3, 1);
	al.SetReferenceSequences(refs);
	int bad = 0, hits_total = 0;
	for (int mode = 0; mode < 2; ++mode) {
		StripedSmithWaterman::Filter filter;
		if (mode == 1) { filter.report_cigar = false; filter.report_begin_position = false; }
		std::vector<std::vector<StripedSmithWaterman::BatchAligner::TopKHit> > hits;
		al.SearchTopK(queries, k, filter, &hits, 20, min_score);
		for (int q = 0; q < nq; ++q) {
			std::vector<std::string> one(refs.size(), queries[(size_t)q]);
			std::vector<int32_t> tix(refs.size());
			for (int t = 0; t < nr; ++t) tix[(size_t)t] = t;
			std::vector<StripedSmithWaterman::Alignment> all;
			std::vector<uint16_t> flags;
			al.AlignPairs(one, tix, filter, &all, 20, &flags);
			std::vector<int> order;
			for (int t = 0; t < nr; ++t) if (all[(size_t)t].sw_score > 0 && all[(size_t)t].sw_score >= min_score) order.push_back(t);
			std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return all[(size_t)a].sw_score > all[(size_t)b].sw_score; });
			if (order.size() > (size_t)k) order.resize((size_t)k);
			const std::vector<StripedSmithWaterman::BatchAligner::TopKHit>& h = hits[(size_t)q];
			if (h.size() != order.size()) { if (++bad <= 5) printf("mode %d query %d: %zu hits, expected %zu\n", mode, q, h.size(), order.size()); continue; }
			for (size_t r = 0; r < h.size(); ++r, ++hits_total) {
				const StripedSmithWaterman::Alignment& e = all[(size_t)order[r]];
				const StripedSmithWaterman::Alignment& g = h[r].alignment;
				const bool same = h[r].target == order[r] && h[r].flag == flags[(size_t)order[r]] && e.sw_score == g.sw_score &&
				                  e.sw_score_next_best == g.sw_score_next_best && e.ref_begin == g.ref_begin && e.ref_end == g.ref_end &&
				                  e.query_begin == g.query_begin && e.query_end == g.query_end && e.ref_end_next_best == g.ref_end_next_best &&
				                  e.mismatches == g.mismatches && e.cigar_string == g.cigar_string && e.cigar == g.cigar;
				if (!same && ++bad <= 5)
					printf("mode %d query %d rank %zu: expected reference %d score %u '%s', got reference %d score %u '%s'\n", mode, q, r, order[r], e.sw_score,
					       e.cigar_string.c_str(), h[r].target, g.sw_score, g.cigar_string.c_str());
			}
		}
	}
	if (bad) { printf("%d differences\n", bad); return 1; }
	printf("ok %d\n", hits_total);
	return 0;
}
