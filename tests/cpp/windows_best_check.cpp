// tests/cpp/windows_best_check.cpp -- TEST INFRASTRUCTURE.  BatchAligner::AlignWindowsBest (include/ssw_gpu_cpp.h) against
// BatchAligner::AlignWindows over ALL candidates followed by the selection rule on the host: per read the chosen candidate, the runner-up
// and its score, the eligible count, and every field of the winner's Alignment (cigar vector and string included) must be equal; a read
// planted in one of its candidates must choose it; with rebase = true the three reference positions move by the winner's begin.
// Usage: windows_best_check [reads] [references]   -> prints "ok <reads>" or the first differences; exit code 0 / 1.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "ssw_gpu_cpp.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 11); }

typedef StripedSmithWaterman::Alignment Aln;
typedef StripedSmithWaterman::BatchAligner::Window Win;
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
	const int nq = argc > 1 ? atoi(argv[1]) : 16, nr = argc > 2 && atoi(argv[2]) > 1 ? atoi(argv[2]) : 3;      // (two references at the least: decoys)
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
	std::vector<int> planted;
	for (int i = 0; i < nq; ++i) {
		const int nc = i == 2 ? 0 : 1 + (int)(rnd() % 6);      // read 2 has no candidate at all
		std::vector<Win> list;
		for (int k = 0; k < nc; ++k) {
			Win w;
			w.reference = (int32_t)(rnd() % (unsigned)nr);
			w.length = 80 + (int32_t)(rnd() % 200);
			w.begin = (int64_t)(rnd() % (unsigned)(refs[(size_t)w.reference].size() - (size_t)w.length + 1));
			list.push_back(w);
		}
		std::string q;
		int pl = -1;
		if (nc > 0) {
			pl = (int)(rnd() % (unsigned)nc);
			for (int k = 0; k < nc; ++k)      // decoys lie on other references than the planted window: none of them can hold the read too
				while (k != pl && list[(size_t)k].reference == list[(size_t)pl].reference) {
					Win& d = list[(size_t)k];
					d.reference = (int32_t)(rnd() % (unsigned)nr);
					d.begin = (int64_t)(rnd() % (unsigned)(refs[(size_t)d.reference].size() - (size_t)d.length + 1));
				}
			const Win w = list[(size_t)pl];
			const std::string win = refs[(size_t)w.reference].substr((size_t)w.begin, (size_t)w.length);
			const int L = 40 + (int)(rnd() % 30), p = (int)(rnd() % (unsigned)(win.size() - (size_t)L + 1));
			q = win.substr((size_t)p, (size_t)L);
			if (i % 5 == 1) q[q.size() / 2] = q[q.size() / 2] == 'A' ? 'C' : 'A';
			if (i % 4 == 3 && nc > 1) {      // the planted window twice: the lower index wins, the other one is the runner-up with the same score
				const int other = (pl + 1) % nc;
				list[(size_t)other] = w;
				if (other < pl) pl = other;
			}
		} else for (int k = 0; k < 50; ++k) q += acgt[rnd() % 4];
		queries.push_back(q); cands.push_back(list); planted.push_back(pl);
		for (size_t k = 0; k < list.size(); ++k) { flat_q.push_back(q); flat_w.push_back(list[k]); }
	}
	StripedSmithWaterman::BatchAligner al(2, 2, 3, 1);
	al.SetReferenceSequences(refs);
	int bad = 0;
	for (int mode = 0; mode < 2; ++mode) {
		StripedSmithWaterman::Filter filter;
		if (mode == 1) { filter.report_cigar = false; filter.report_begin_position = false; }
		std::vector<Aln> got, got_rebased, all;
		std::vector<Best> best, best_rebased;
		std::vector<uint16_t> aflags;
		al.AlignWindowsBest(queries, cands, filter, &got, &best, 20, 1);
		al.AlignWindowsBest(queries, cands, filter, &got_rebased, &best_rebased, 20, 1, true);
		al.AlignWindows(flat_q, flat_w, filter, &all, 20, false, &aflags);
		size_t c0 = 0;
		for (int i = 0; i < nq; ++i) {
			const size_t nc = cands[(size_t)i].size();
			int b = -1, s = -1, ne = 0;
			for (size_t k = 0; k < nc; ++k) {      // sw_score descending, then index ascending
				const unsigned sc = all[c0 + k].sw_score;
				if (sc < 1) continue;
				++ne;
				if (b < 0 || sc > all[c0 + (size_t)b].sw_score) { s = b; b = (int)k; }
				else if (s < 0 || sc > all[c0 + (size_t)s].sw_score) s = (int)k;
			}
			const Best& g = best[(size_t)i];
			bool ok = g.candidate == b && g.runner_up == s && g.eligible == ne && g.runner_up_score == (s >= 0 ? all[c0 + (size_t)s].sw_score : 0) &&
			          g.candidate == planted[(size_t)i] && best_rebased[(size_t)i].candidate == b;
			if (ok && b >= 0)
				ok = same(all[c0 + (size_t)b], got[(size_t)i], 0) && g.flag == aflags[c0 + (size_t)b] &&
				     same(all[c0 + (size_t)b], got_rebased[(size_t)i], (int)cands[(size_t)i][(size_t)b].begin);
			if (ok && b < 0) ok = same(Aln(), got[(size_t)i], 0);
			if (!ok && ++bad <= 5)
				printf("mode %d read %d (%zu candidates, planted %d): expected best %d second %d eligible %d, got best %d second %d (score %u) eligible %d, score %u '%s'\n",
				       mode, i, nc, planted[(size_t)i], b, s, ne, g.candidate, g.runner_up, g.runner_up_score, g.eligible, got[(size_t)i].sw_score,
				       got[(size_t)i].cigar_string.c_str());
			c0 += nc;
		}
	}
	bool threw = false;      // a candidate window that leaves its reference is refused, not clamped
	try {
		std::vector<std::vector<Win> > c1(1, std::vector<Win>(1, flat_w[0]));
		c1[0][0].begin = (int64_t)refs[(size_t)c1[0][0].reference].size();
		std::vector<std::string> q1(1, queries[0]);
		std::vector<Aln> out; std::vector<Best> ob;
		al.AlignWindowsBest(q1, c1, StripedSmithWaterman::Filter(), &out, &ob, 20);
	} catch (const std::runtime_error&) { threw = true; }
	if (!threw) { printf("a window beyond its reference's end was accepted\n"); ++bad; }
	if (bad) { printf("%d differences\n", bad); return 1; }
	printf("ok %d\n", nq);
	return 0;
}
