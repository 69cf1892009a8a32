// tests/cpp/mates_model_check.cpp -- TEST INFRASTRUCTURE.  BatchAligner::AlignWindowsMates (include/ssw_gpu_cpp.h) with an insert_penalty
// table (the pair model of include/ssw_gpu.h) against BatchAligner::AlignWindows over ALL candidates -- a candidate on the reverse strand
// as the reverse-complemented query string -- followed by the model's rule on the host: a proper combination of span D pays
// insert_penalty[D - min_insert], an improper one unpaired_penalty.  Per fragment the two candidate indices, the eligible counts, score,
// second score, proper count and proper flag, per read every field of the Alignment must be equal.  All three library orientations; a
// table that ignores unpaired_penalty (entries above it); nullptr gives what the call without the argument gives; a table of the wrong
// length throws.
// Usage: mates_model_check [fragments] [references]   -> prints "ok <fragments>" or the first differences; exit code 0 / 1.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>

#include "ssw_gpu_cpp.h"

static unsigned long long rng_state = 0xD1B54A32D192ED03ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 11); }

typedef StripedSmithWaterman::Alignment Aln;
typedef StripedSmithWaterman::BatchAligner::Window Win;
typedef StripedSmithWaterman::BatchAligner::MateWindow MWin;
typedef StripedSmithWaterman::BatchAligner::MatePair Pair;

static bool same(const Aln& e, const Aln& g)
{
	return e.sw_score == g.sw_score && e.sw_score_next_best == g.sw_score_next_best && e.ref_begin == g.ref_begin && e.ref_end == g.ref_end &&
	       e.query_begin == g.query_begin && e.query_end == g.query_end && e.ref_end_next_best == g.ref_end_next_best &&
	       e.mismatches == g.mismatches && e.cigar_string == g.cigar_string && e.cigar == g.cigar;
}

static bool same_pair(const Pair& x, const Pair& y)
{
	return x.candidate1 == y.candidate1 && x.candidate2 == y.candidate2 && x.eligible1 == y.eligible1 && x.eligible2 == y.eligible2 &&
	       x.score == y.score && x.second_score == y.second_score && x.proper_count == y.proper_count && x.proper == y.proper &&
	       x.flag1 == y.flag1 && x.flag2 == y.flag2;
}

static std::string revcomp(const std::string& s)      // A/C/G/T complemented, everything else kept
{
	std::string r(s.rbegin(), s.rend());
	for (size_t i = 0; i < r.size(); ++i) r[i] = r[i] == 'A' ? 'T' : r[i] == 'C' ? 'G' : r[i] == 'G' ? 'C' : r[i] == 'T' ? 'A' : r[i];
	return r;
}

struct Comb { int s, a, b; bool proper; };
static bool before(const Comb& x, const Comb& y) { return x.s != y.s ? x.s > y.s : x.a != y.a ? x.a < y.a : x.b < y.b; }

int main(int argc, char** argv)
{
	const int nf = argc > 1 ? atoi(argv[1]) : 16, nr = argc > 2 && atoi(argv[2]) > 1 ? atoi(argv[2]) : 2;
	const char acgt[] = "ACGT";
	std::vector<std::string> refs;
	for (int t = 0; t < nr; ++t) {
		std::string s;
		const int L = 1500 + (int)(rnd() % 500) + t;
		for (int i = 0; i < L; ++i) s += acgt[rnd() % 4];
		refs.push_back(s);
	}
	// fragment f: 150..400 columns of one reference, one mate from either end, on the strands of an FR (f % 3 == 0), RF (1) or FF (2; every
	// other one on the minus strand with mate 2 upstream) library; the true locus is always among the candidates, so that proper pairs exist
	std::vector<std::string> reads, flat_q;
	std::vector<std::vector<MWin> > cands;
	std::vector<Win> flat_w;
	std::vector<size_t> first;      // first flat candidate of every read
	for (int f = 0; f < nf; ++f) {
		const int t = (int)(rnd() % (unsigned)nr), ins = 150 + (int)(rnd() % 251);
		const int s = (int)(rnd() % (unsigned)(refs[(size_t)t].size() - (size_t)ins + 1));
		const int len[2] = { 40 + (int)(rnd() % 40), 40 + (int)(rnd() % 40) };
		const int home[2] = { s, s + ins - len[1] };
		bool minus[2];
		const int lib = f % 3, flip = (int)(rnd() % 2);
		if (lib == 0) { minus[0] = false; minus[1] = true; } else if (lib == 1) { minus[0] = true; minus[1] = false; } else minus[0] = minus[1] = (f % 2) != 0;
		const int end_of_mate1 = lib == 2 ? (minus[0] ? 1 : 0) : flip;
		for (int h = 0; h < 2; ++h) {
			const int e = h == 0 ? end_of_mate1 : 1 - end_of_mate1;
			std::string q = refs[(size_t)t].substr((size_t)home[e], (size_t)len[e]);
			if ((2 * f + h) % 5 == 1) q[q.size() / 2] = q[q.size() / 2] == 'A' ? 'C' : 'A';
			const std::string stored = minus[e] ? revcomp(q) : q;
			const int nc = f == 2 ? 0 : f == 4 && h == 1 ? 0 : 1 + (int)(rnd() % 5);      // fragment 2 has no candidate, fragment 4 none for mate 2
			std::vector<MWin> list;
			for (int c = 0; c < nc; ++c) {
				MWin w;
				w.length = 80 + (int32_t)(rnd() % 170);
				if (c == 0 || rnd() % 2) {
					w.reference = t;
					long b = (long)home[e] - (long)w.length + len[e] + (long)(rnd() % (unsigned)(w.length - len[e] + 1));      // the locus lies inside
					const long last = (long)refs[(size_t)t].size() - w.length;
					w.begin = b < 0 ? 0 : b > last ? last : b;
				} else {
					w.reference = (int32_t)(rnd() % (unsigned)nr);
					w.begin = (int64_t)(rnd() % (unsigned)(refs[(size_t)w.reference].size() - (size_t)w.length + 1));
				}
				w.reverse = c == 0 || rnd() % 4 ? minus[e] : !minus[e];
				list.push_back(w);
			}
			if (nc > 2) std::swap(list[0], list[(size_t)nc - 1]);      // (the true locus is not always the first position)
			first.push_back(flat_q.size());
			reads.push_back(stored); cands.push_back(list);
			for (size_t c = 0; c < list.size(); ++c) {
				Win w; w.reference = list[c].reference; w.begin = list[c].begin; w.length = list[c].length;
				flat_q.push_back(list[c].reverse ? revcomp(stored) : stored); flat_w.push_back(w);
			}
		}
	}
	StripedSmithWaterman::BatchAligner al(2, 2, 3, 1);
	al.SetReferenceSequences(refs);
	int bad = 0, proper_seen[3] = { 0, 0, 0 }, changed = 0;
	const int mn = 100, mx = 500, pen = 25;
	// two tables: a bowl around span 275, capped at 40 -- above unpaired_penalty at the rim --, and one whose neighbours all differ
	std::vector<std::vector<uint16_t> > tables(2, std::vector<uint16_t>((size_t)(mx - mn + 1)));
	for (int i = 0; i <= mx - mn; ++i) {
		const int d = abs(mn + i - 275);
		tables[0][(size_t)i] = (uint16_t)std::min(40, d * d / 400);
		tables[1][(size_t)i] = (uint16_t)(1 + (7 * i) % 13);
	}
	StripedSmithWaterman::Filter filter;
	std::vector<Aln> all;
	al.AlignWindows(flat_q, flat_w, filter, &all, 20, false);
	for (int o = 0; o < 3; ++o) {
		std::vector<Aln> base, viaNull;
		std::vector<Pair> pbase, pviaNull;
		al.AlignWindowsMates(reads, cands, filter, &base, &pbase, 20, mn, mx, pen, 0, o);
		al.AlignWindowsMates(reads, cands, filter, &viaNull, &pviaNull, 20, mn, mx, pen, 0, o, false, nullptr);
		for (int f = 0; f < nf; ++f)
			if (!same_pair(pbase[(size_t)f], pviaNull[(size_t)f]) || !same(base[2 * (size_t)f], viaNull[2 * (size_t)f]) ||
			    !same(base[2 * (size_t)f + 1], viaNull[2 * (size_t)f + 1])) {
				if (++bad <= 5) printf("orientation %d fragment %d: nullptr differs from the call without the argument\n", o, f);
			}
		for (size_t ti = 0; ti < tables.size(); ++ti)
			for (int v = 0; v < 2; ++v) {
				const std::vector<uint16_t>& table = tables[ti];
				const int min_score = v ? 60 : 0;
				std::vector<Aln> got;
				std::vector<Pair> pairs;
				al.AlignWindowsMates(reads, cands, filter, &got, &pairs, 20, mn, mx, pen, min_score, o, false, &table);
				for (int f = 0; f < nf; ++f) {
					const size_t r1 = 2 * (size_t)f, r2 = r1 + 1;
					std::vector<int> e1, e2;
					for (size_t c = 0; c < cands[r1].size(); ++c) if (all[first[r1] + c].sw_score >= 1 && (int)all[first[r1] + c].sw_score >= min_score) e1.push_back((int)c);
					for (size_t c = 0; c < cands[r2].size(); ++c) if (all[first[r2] + c].sw_score >= 1 && (int)all[first[r2] + c].sw_score >= min_score) e2.push_back((int)c);
					int p1 = -1, p2 = -1, score = 0, second = 0, npr = 0;
					bool pr = false;
					if (!e1.empty() && !e2.empty()) {
						std::vector<Comb> comb;
						for (size_t x = 0; x < e1.size(); ++x)
							for (size_t y = 0; y < e2.size(); ++y) {
								const MWin& a = cands[r1][(size_t)e1[x]]; const MWin& b = cands[r2][(size_t)e2[y]];
								const Aln& ra = all[first[r1] + (size_t)e1[x]]; const Aln& rb = all[first[r2] + (size_t)e2[y]];
								const long long Ea = a.begin + ra.ref_end, Eb = b.begin + rb.ref_end;
								const long long Ba = Ea - (long long)reads[r1].size() + 1, Bb = Eb - (long long)reads[r2].size() + 1;
								bool proper = a.reference == b.reference && (o == 2 ? a.reverse == b.reverse : a.reverse != b.reverse);
								long long D = 0;
								if (o == 0) D = a.reverse ? Ea - Bb + 1 : Eb - Ba + 1;           // E(minus) - B(plus) + 1
								else if (o == 1) D = a.reverse ? Eb - Ba + 1 : Ea - Bb + 1;      // E(plus) - B(minus) + 1
								else D = a.reverse ? Ea - Bb + 1 : Eb - Ba + 1;                  // both minus: mate 2 upstream; both plus: mate 1
								proper = proper && D >= mn && D <= mx;
								Comb k; k.s = (int)ra.sw_score + (int)rb.sw_score - (proper ? (int)table[(size_t)(D - mn)] : pen); k.a = e1[x]; k.b = e2[y]; k.proper = proper;
								comb.push_back(k); npr += proper;
							}
						std::sort(comb.begin(), comb.end(), before);
						p1 = comb[0].a; p2 = comb[0].b; score = comb[0].s; pr = comb[0].proper; second = comb.size() > 1 ? comb[1].s : 0;
					} else if (!e1.empty() || !e2.empty()) {
						const std::vector<int>& e = e1.empty() ? e2 : e1; const size_t r = e1.empty() ? r2 : r1;
						std::vector<std::pair<int, int> > order;
						for (size_t x = 0; x < e.size(); ++x) order.push_back(std::make_pair(-(int)all[first[r] + (size_t)e[x]].sw_score, e[x]));
						std::sort(order.begin(), order.end());
						(e1.empty() ? p2 : p1) = order[0].second; score = -order[0].first; second = order.size() > 1 ? -order[1].first : 0;
					}
					const Pair& g = pairs[(size_t)f];
					bool ok = g.candidate1 == p1 && g.candidate2 == p2 && g.eligible1 == (int)e1.size() && g.eligible2 == (int)e2.size() && g.score == score &&
					          g.second_score == second && g.proper_count == npr && g.proper == pr;
					for (int h = 0; ok && h < 2; ++h) {
						const size_t r = r1 + (size_t)h;
						const int pos = h ? p2 : p1;
						ok = pos < 0 ? same(Aln(), got[r]) : same(all[first[r] + (size_t)pos], got[r]);
					}
					if (pr) ++proper_seen[o];
					if (v == 0 && (g.score != pbase[(size_t)f].score || g.candidate1 != pbase[(size_t)f].candidate1 || g.candidate2 != pbase[(size_t)f].candidate2)) ++changed;
					if (!ok && ++bad <= 5)
						printf("orientation %d table %zu min_score %d fragment %d: expected (%d, %d) score %d second %d proper %d of %d; got (%d, %d) score %d second %d proper %d of %d\n",
						       o, ti, min_score, f, p1, p2, score, second, (int)pr, npr, g.candidate1, g.candidate2, g.score, g.second_score, (int)g.proper, g.proper_count);
				}
			}
	}
	if (nf >= 12 && !(proper_seen[0] && proper_seen[1] && proper_seen[2] && changed)) {
		printf("the case is too weak: proper pairs per orientation %d %d %d, fragments the table changes %d\n", proper_seen[0], proper_seen[1], proper_seen[2], changed);
		++bad;
	}
	int threw = 0;      // a table one entry short, one entry long
	for (int what = 0; what < 2; ++what)
		try {
			std::vector<uint16_t> t2((size_t)(mx - mn + (what ? 2 : 0)), 1);
			std::vector<Aln> out; std::vector<Pair> op;
			al.AlignWindowsMates(reads, cands, filter, &out, &op, 20, mn, mx, pen, 0, 0, false, &t2);
		} catch (const std::runtime_error&) { ++threw; }
	if (threw != 2) { printf("a table of the wrong length was accepted (%d of 2 refused)\n", threw); ++bad; }
	if (bad) { printf("%d differences\n", bad); return 1; }
	printf("ok %d\n", nf);
	return 0;
}
