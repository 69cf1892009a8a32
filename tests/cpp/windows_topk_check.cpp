// tests/cpp/windows_topk_check.cpp -- TEST INFRASTRUCTURE.  BatchAligner::AlignWindowsTopK (include/ssw_gpu_cpp.h) against
// BatchAligner::AlignWindows over ALL candidates followed by the ranking rule on the host (sw_score descending, then index ascending,
// rank r >= 1 only while its score >= score(rank 0) - max_drop): per read the reported candidates in order, the eligible count, the
// s_align flag and every field of every reported Alignment (cigar vector and string included) must be equal; with rebase = true the
// three reference positions move by the chosen candidate's begin; k = 1 must agree with AlignWindowsBest.
// Usage: windows_topk_check [reads] [references]   -> prints "ok <reads>" or the first differences; exit code 0 / 1.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>

#include "ssw_gpu_cpp.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 11); }

typedef StripedSmithWaterman::Alignment Aln;
typedef StripedSmithWaterman::BatchAligner::Window Win;
typedef StripedSmithWaterman::BatchAligner::WindowHit Hit;
typedef StripedSmithWaterman::BatchAligner::BestWindow Best;

static bool same(const Aln& e, const Aln& g, int shift)
{
	return e.sw_score == g.sw_score && e.sw_score_next_best == g.sw_score_next_best && e.ref_begin + (e.ref_begin >= 0 ? shift : 0) == g.ref_begin &&
	       e.ref_end + (e.ref_end >= 0 ? shift : 0) == g.ref_end && e.query_begin == g.query_begin && e.query_end == g.query_end &&
	       e.ref_end_next_best + (e.ref_end_next_best >= 0 ? shift : 0) == g.ref_end_next_best && e.mismatches == g.mismatches &&
	       e.cigar_string == g.cigar_string && e.cigar == g.cigar;
}

int main(int argc, char** argv)
{
	const int nq = argc > 1 ? atoi(argv[1]) : 16, nr = argc > 2 && atoi(argv[2]) > 1 ? atoi(argv[2]) : 3;
	const char acgt[] = "ACGT";
	std::vector<std::string> refs;
	for (int t = 0; t < nr; ++t) {
		std::string s;
		const int L = 600 + (int)(rnd() % 500) + t;
		for (int i = 0; i < L; ++i) s += acgt[rnd() % 4];
		refs.push_back(s);
	}
	std::vector<std::string> queries, flat_q;
	std::vector<std::vector<Win> > cands;
	std::vector<Win> flat_w;
	for (int i = 0; i < nq; ++i) {
		// the read lies on reference t at [s, s + L); about half of its candidates overlap it by some amount, one of them twice (a tie)
		const int t = (int)(rnd() % (unsigned)nr), L = 40 + (int)(rnd() % 30);
		const int s = (int)(rnd() % (unsigned)(refs[(size_t)t].size() - (size_t)L + 1));
		std::string q = refs[(size_t)t].substr((size_t)s, (size_t)L);
		if (i % 5 == 1) q[q.size() / 2] = q[q.size() / 2] == 'A' ? 'C' : 'A';
		const int nc = i == 2 ? 0 : 1 + (int)(rnd() % 9);      // read 2 has no candidate at all
		std::vector<Win> list;
		for (int c = 0; c < nc; ++c) {
			Win w;
			w.length = 80 + (int32_t)(rnd() % 200);
			if (rnd() % 2) {
				w.reference = t;
				long b = (long)s - (long)w.length + L / 4 + (long)(rnd() % (unsigned)(w.length + L / 2));
				const long last = (long)refs[(size_t)t].size() - w.length;
				w.begin = b < 0 ? 0 : b > last ? last : b;
			} else {
				w.reference = (int32_t)(rnd() % (unsigned)nr);
				w.begin = (int64_t)(rnd() % (unsigned)(refs[(size_t)w.reference].size() - (size_t)w.length + 1));
			}
			list.push_back(w);
		}
		if (i % 4 == 3 && nc > 2) list[(size_t)nc - 1] = list[0];
		queries.push_back(q); cands.push_back(list);
		for (size_t c = 0; c < list.size(); ++c) { flat_q.push_back(q); flat_w.push_back(list[c]); }
	}
	StripedSmithWaterman::BatchAligner al(2, 2, 3, 1);
	al.SetReferenceSequences(refs);
	int bad = 0;
	const int ks[3] = { 1, 3, 8 }, drops[3] = { -1, 0, 25 };
	for (int mode = 0; mode < 2; ++mode) {
		StripedSmithWaterman::Filter filter;
		if (mode == 1) { filter.report_cigar = false; filter.report_begin_position = false; }
		std::vector<Aln> all;
		std::vector<uint16_t> aflags;
		al.AlignWindows(flat_q, flat_w, filter, &all, 20, false, &aflags);
		for (int v = 0; v < 3; ++v) {
			const int k = ks[v], drop = drops[v], min_score = v == 2 ? 20 : 1;
			std::vector<std::vector<Aln> > got, got_rebased;
			std::vector<std::vector<Hit> > hits, hits_rebased;
			std::vector<int32_t> elig, elig_rebased;
			al.AlignWindowsTopK(queries, cands, filter, k, &got, &hits, &elig, 20, min_score, drop);
			al.AlignWindowsTopK(queries, cands, filter, k, &got_rebased, &hits_rebased, &elig_rebased, 20, min_score, drop, true);
			std::vector<Aln> bgot; std::vector<Best> best;
			if (k == 1) al.AlignWindowsBest(queries, cands, filter, &bgot, &best, 20, min_score);
			size_t c0 = 0;
			for (int i = 0; i < nq; ++i) {
				const size_t nc = cands[(size_t)i].size();
				std::vector<std::pair<int, int> > order;      // (-score, index): ascending = the ranking
				for (size_t c = 0; c < nc; ++c)
					if (all[c0 + c].sw_score >= 1 && (int)all[c0 + c].sw_score >= min_score) order.push_back(std::make_pair(-(int)all[c0 + c].sw_score, (int)c));
				std::sort(order.begin(), order.end());
				size_t want = std::min(order.size(), (size_t)k);
				if (drop >= 0) for (size_t r = 1; r < want; ++r) if (-order[r].first < -order[0].first - drop) { want = r; break; }
				bool ok = (size_t)elig[(size_t)i] == order.size() && got[(size_t)i].size() == want && hits[(size_t)i].size() == want &&
				          got_rebased[(size_t)i].size() == want && elig_rebased[(size_t)i] == elig[(size_t)i];
				for (size_t r = 0; ok && r < want; ++r) {
					const size_t c = (size_t)order[r].second;
					ok = hits[(size_t)i][r].candidate == (int)c && hits_rebased[(size_t)i][r].candidate == (int)c && hits[(size_t)i][r].flag == aflags[c0 + c] &&
					     same(all[c0 + c], got[(size_t)i][r], 0) && same(all[c0 + c], got_rebased[(size_t)i][r], (int)cands[(size_t)i][c].begin);
				}
				if (ok && k == 1)
					ok = best[(size_t)i].candidate == (want ? hits[(size_t)i][0].candidate : -1) && best[(size_t)i].eligible == elig[(size_t)i] &&
					     (!want || same(bgot[(size_t)i], got[(size_t)i][0], 0));
				if (!ok && ++bad <= 5)
					printf("mode %d k %d max_drop %d read %d (%zu candidates): expected %zu ranks of %zu eligible (first %d), got %zu of %d (first %d)\n", mode, k, drop, i, nc,
					       want, order.size(), want ? order[0].second : -1, got[(size_t)i].size(), elig[(size_t)i], hits[(size_t)i].empty() ? -1 : hits[(size_t)i][0].candidate);
				c0 += nc;
			}
		}
	}
	int threw = 0;      // a candidate window that leaves its reference is refused, not clamped; so is k = 0
	for (int what = 0; what < 2; ++what)
		try {
			std::vector<std::vector<Win> > c1(1, std::vector<Win>(1, flat_w[0]));
			if (what == 0) c1[0][0].begin = (int64_t)refs[(size_t)c1[0][0].reference].size();
			std::vector<std::string> q1(1, queries[0]);
			std::vector<std::vector<Aln> > out; std::vector<std::vector<Hit> > oh; std::vector<int32_t> oe;
			al.AlignWindowsTopK(q1, c1, StripedSmithWaterman::Filter(), what == 0 ? 2 : 0, &out, &oh, &oe, 20);
		} catch (const std::runtime_error&) { ++threw; }
	if (threw != 2) { printf("a window beyond its reference's end, or k = 0, was accepted\n"); ++bad; }
	if (bad) { printf("%d differences\n", bad); return 1; }
	printf("ok %d\n", nq);
	return 0;
}
