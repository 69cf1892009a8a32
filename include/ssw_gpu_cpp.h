// ssw_gpu_cpp.h -- batched counterpart of the reference's C++ wrapper (mengyao/Complete-Striped-Smith-Waterman-Library
// src/ssw_cpp.h / ssw_cpp.cpp), header-only, over the batch C-ABI of libssw.so (include/ssw_gpu.h).
//
// The reference's StripedSmithWaterman::Aligner::Align (ssw_cpp.cpp:319-357) aligns ONE query per call: ssw_init + ssw_align +
// ConvertAlignment + CalculateNumberMismatch.  A caller that loops over reads keeps working unchanged on libssw.so (the drop-in
// path), but every call is a synchronous round trip to the GPU.  BatchAligner is the same operation for a whole vector of
// queries against the reference sequence(s) set once: ONE ssw_gpu_align_batch call, and the same Alignment records --
// sw_score, sw_score_next_best, ref/query begin/end, ref_end_next_best, mismatches, cigar / cigar_string with soft clips and
// '=' / 'X' runs -- as Aligner::Align returns for each query (tests/cpp/batch_check.cpp compares the two on the MI355X).
//
// Alignment and Filter are the reference's structs (ssw_cpp.h:15-63): when the reference header was included first they are
// used as they are; otherwise the same two structs are declared here, field for field, so that existing code compiles either way.
#ifndef SSW_GPU_CPP_H
#define SSW_GPU_CPP_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "ssw.h"
#include "ssw_gpu.h"

#ifndef COMPLETE_STRIPED_SMITH_WATERMAN_CPP_H_
namespace StripedSmithWaterman {
struct Alignment {
  uint16_t sw_score;
  uint16_t sw_score_next_best;
  int32_t ref_begin;
  int32_t ref_end;
  int32_t query_begin;
  int32_t query_end;
  int32_t ref_end_next_best;
  int32_t mismatches;
  std::string cigar_string;
  std::vector<uint32_t> cigar;
  Alignment() : sw_score(0), sw_score_next_best(0), ref_begin(0), ref_end(0), query_begin(0), query_end(0), ref_end_next_best(0), mismatches(0) {}
  void Clear() { *this = Alignment(); }
};
struct Filter {
  bool report_begin_position;
  bool report_cigar;
  uint16_t score_filter;
  uint16_t distance_filter;
  Filter() : report_begin_position(true), report_cigar(true), score_filter(0), distance_filter(32767) {}
  Filter(const bool& pos, const bool& cigar, const uint16_t& score, const uint16_t& dis)
      : report_begin_position(pos), report_cigar(cigar), score_filter(score), distance_filter(dis) {}
};
}  // namespace StripedSmithWaterman
#endif

namespace StripedSmithWaterman {

class BatchAligner {
 public:
  // default scoring of the reference's Aligner(): match 2, mismatch 2, gap open 3, gap extension 1, A/C/G/T/N
  BatchAligner(int device = 0) : ctx_(0), targets_(0), n_targets_(0), gap_open_(3), gap_extend_(1) {
    ctx_ = ssw_gpu_open(device);
    if (!ctx_) throw std::runtime_error(std::string("ssw_gpu_open: ") + ssw_gpu_last_error(0));
    SetDnaScores(2, 2);
  }
  BatchAligner(uint8_t match_score, uint8_t mismatch_penalty, uint8_t gap_opening_penalty, uint8_t gap_extending_penalty, int device = 0)
      : ctx_(0), targets_(0), n_targets_(0), gap_open_(gap_opening_penalty), gap_extend_(gap_extending_penalty) {
    ctx_ = ssw_gpu_open(device);
    if (!ctx_) throw std::runtime_error(std::string("ssw_gpu_open: ") + ssw_gpu_last_error(0));
    SetDnaScores(match_score, mismatch_penalty);
  }
  // user matrices, as Aligner(score_matrix, score_matrix_size, translation_matrix, translation_matrix_size) (ssw_cpp.cpp:216-231)
  BatchAligner(const int8_t* score_matrix, int score_matrix_size, const int8_t* translation_matrix, int translation_matrix_size, int device = 0)
      : ctx_(0), targets_(0), n_targets_(0), gap_open_(3), gap_extend_(1) {
    ctx_ = ssw_gpu_open(device);
    if (!ctx_) throw std::runtime_error(std::string("ssw_gpu_open: ") + ssw_gpu_last_error(0));
    matrix_size_ = score_matrix_size;
    matrix_.assign(score_matrix, score_matrix + score_matrix_size * score_matrix_size);
    table_.assign(128, 0);
    for (int i = 0; i < translation_matrix_size && i < 128; ++i) table_[i] = translation_matrix[i];
  }
  ~BatchAligner() {
    if (targets_) ssw_gpu_seqs_free(targets_);
    if (ctx_) ssw_gpu_close(ctx_);
  }
  void SetGapPenalty(uint8_t opening, uint8_t extending) { gap_open_ = opening; gap_extend_ = extending; }

  // the reference sequence(s), translated on the device and kept in HBM (Aligner::SetReferenceSequence keeps its translation on the host)
  int SetReferenceSequence(const char* seq, int length) {
    std::vector<std::string> one(1, std::string(seq, seq + length));
    return SetReferenceSequences(one);
  }
  int SetReferenceSequences(const std::vector<std::string>& refs) {
    if (targets_) { ssw_gpu_seqs_free(targets_); targets_ = 0; }
    std::string text; std::vector<int64_t> off(1, 0);
    for (size_t i = 0; i < refs.size(); ++i) { text += refs[i]; off.push_back((int64_t)text.size()); }
    targets_ = ssw_gpu_seqs_upload_ascii(ctx_, text.data(), off.data(), (int32_t)refs.size(), table_.data());
    if (!targets_) throw std::runtime_error(std::string("ssw_gpu_seqs_upload_ascii: ") + ssw_gpu_last_error(ctx_));
    ref_codes_.resize(text.size()); ref_off_ = off; n_targets_ = (int)refs.size();
    for (size_t i = 0; i < text.size(); ++i) ref_codes_[i] = table_[(unsigned char)text[i] & 127];
    return n_targets_;
  }

  // Every query against reference `target` (default: the first / only one): alignments[i] is what Aligner::Align(queries[i], filter,
  // &alignments[i], maskLen) gives; flags[i] (optional) its return value (s_align.flag).  maskLen < 15 is raised to 15 like there.
  void Align(const std::vector<std::string>& queries, const Filter& filter, std::vector<Alignment>* alignments, int32_t maskLen,
             std::vector<uint16_t>* flags = 0, int target = 0) const {
    if (!targets_ || target < 0 || target >= n_targets_) throw std::runtime_error("BatchAligner::Align: no such reference sequence");
    const int32_t nq = (int32_t)queries.size();
    alignments->assign(queries.size(), Alignment());
    if (flags) flags->assign(queries.size(), 0);
    if (nq == 0) return;
    std::string text; std::vector<int64_t> off(1, 0);
    for (int32_t i = 0; i < nq; ++i) { text += queries[i]; off.push_back((int64_t)text.size()); }
    ssw_gpu_seqs* Q = ssw_gpu_seqs_upload_ascii(ctx_, text.data(), off.data(), nq, table_.data());
    if (!Q) throw std::runtime_error(std::string("ssw_gpu_seqs_upload_ascii: ") + ssw_gpu_last_error(ctx_));
    ssw_gpu_params p; memset(&p, 0, sizeof p);
    p.mat = matrix_.data(); p.n = matrix_size_; p.gapO = gap_open_; p.gapE = gap_extend_;
    p.flag = (uint8_t)((filter.report_begin_position ? 0x08 : 0) | (filter.report_cigar ? 0x0f : 0));      // SetFlag, ssw_cpp.cpp:204-211
    p.filters = filter.score_filter; p.filterd = filter.distance_filter; p.maskLen = std::max(maskLen, 15); p.score_size = 2;
    std::vector<ssw_gpu_result> res((size_t)nq);
    uint32_t* pool = 0; int64_t words = 0;
    const int rc = ssw_gpu_align_batch(ctx_, Q, targets_, target, 1, &p, res.data(), &pool, &words);
    ssw_gpu_seqs_free(Q);
    if (rc != 0) { free(pool); throw std::runtime_error(std::string("ssw_gpu_align_batch: ") + (rc == SSW_GPU_BUSY ? ssw_gpu_strerror(rc) : ssw_gpu_last_error(ctx_))); }
    const int8_t* ref = ref_codes_.data() + ref_off_[(size_t)target];
    for (int32_t i = 0; i < nq; ++i) {
      const ssw_gpu_result& r = res[(size_t)i];
      Alignment& a = (*alignments)[(size_t)i];
      a.sw_score = r.score1; a.sw_score_next_best = r.score2; a.ref_begin = r.ref_begin1; a.ref_end = r.ref_end1;
      a.query_begin = r.read_begin1; a.query_end = r.read_end1; a.ref_end_next_best = r.ref_end2;
      if (flags) (*flags)[(size_t)i] = r.flag;
      const int qlen = (int)queries[(size_t)i].size();
      Expand(a, r.cigarLen > 0 ? pool + r.cigar_off : 0, r.cigarLen, ref, text.data() + off[(size_t)i], qlen);
    }
    free(pool);
  }

  // A mapper's loop as one call: alignments[i] is what Aligner::Align(queries[i], filter, &alignments[i], maskLen) gives against reference
  // target_index_per_query[i] (ssw_gpu_align_pairs); flags[i] (optional) its return value.  maskLen < 15 is raised to 15 like there.
  void AlignPairs(const std::vector<std::string>& queries, const std::vector<int32_t>& target_index_per_query, const Filter& filter,
                  std::vector<Alignment>* alignments, int32_t maskLen, std::vector<uint16_t>* flags = 0) const {
    if (!targets_) throw std::runtime_error("BatchAligner::AlignPairs: no reference sequences");
    if (target_index_per_query.size() != queries.size()) throw std::runtime_error("BatchAligner::AlignPairs: one target index per query");
    const int32_t nq = (int32_t)queries.size();
    for (int32_t i = 0; i < nq; ++i)
      if (target_index_per_query[(size_t)i] < 0 || target_index_per_query[(size_t)i] >= n_targets_) throw std::runtime_error("BatchAligner::AlignPairs: no such reference sequence");
    alignments->assign(queries.size(), Alignment());
    if (flags) flags->assign(queries.size(), 0);
    if (nq == 0) return;
    std::string text; std::vector<int64_t> off(1, 0);
    for (int32_t i = 0; i < nq; ++i) { text += queries[i]; off.push_back((int64_t)text.size()); }
    ssw_gpu_seqs* Q = ssw_gpu_seqs_upload_ascii(ctx_, text.data(), off.data(), nq, table_.data());
    if (!Q) throw std::runtime_error(std::string("ssw_gpu_seqs_upload_ascii: ") + ssw_gpu_last_error(ctx_));
    ssw_gpu_params p; memset(&p, 0, sizeof p);
    p.mat = matrix_.data(); p.n = matrix_size_; p.gapO = gap_open_; p.gapE = gap_extend_;
    p.flag = (uint8_t)((filter.report_begin_position ? 0x08 : 0) | (filter.report_cigar ? 0x0f : 0));
    p.filters = filter.score_filter; p.filterd = filter.distance_filter; p.maskLen = std::max(maskLen, 15); p.score_size = 2;
    std::vector<int32_t> qidx((size_t)nq);
    for (int32_t i = 0; i < nq; ++i) qidx[(size_t)i] = i;
    std::vector<ssw_gpu_result> res((size_t)nq);
    uint32_t* pool = 0; int64_t words = 0;
    const int rc = ssw_gpu_align_pairs(ctx_, Q, targets_, qidx.data(), target_index_per_query.data(), nq, &p, res.data(), &pool, &words);
    ssw_gpu_seqs_free(Q);
    if (rc != 0) { free(pool); throw std::runtime_error(std::string("ssw_gpu_align_pairs: ") + (rc == SSW_GPU_BUSY ? ssw_gpu_strerror(rc) : ssw_gpu_last_error(ctx_))); }
    for (int32_t i = 0; i < nq; ++i) {
      const ssw_gpu_result& r = res[(size_t)i];
      Alignment& a = (*alignments)[(size_t)i];
      a.sw_score = r.score1; a.sw_score_next_best = r.score2; a.ref_begin = r.ref_begin1; a.ref_end = r.ref_end1;
      a.query_begin = r.read_begin1; a.query_end = r.read_end1; a.ref_end_next_best = r.ref_end2;
      if (flags) (*flags)[(size_t)i] = r.flag;
      const int8_t* ref = ref_codes_.data() + ref_off_[(size_t)target_index_per_query[(size_t)i]];
      Expand(a, r.cigarLen > 0 ? pool + r.cigar_off : 0, r.cigarLen, ref, text.data() + off[(size_t)i], (int)queries[(size_t)i].size());
    }
    free(pool);
  }

  // Reads against windows of the resident reference sequences (ssw_gpu_align_windows): alignments[i] is what AlignPairs gives for
  // queries[i] against a reference that consists of residues [begin, begin + length) of reference windows[i].reference -- nothing of the
  // references is copied or uploaded again.  Positions are relative to the window; rebase = true adds windows[i].begin to ref_begin,
  // ref_end and ref_end_next_best where they are >= 0 (reference coordinates).  A window that leaves its reference throws.
  struct Window {
    int32_t reference;
    int64_t begin;
    int32_t length;
  };
  void AlignWindows(const std::vector<std::string>& queries, const std::vector<Window>& windows, const Filter& filter,
                    std::vector<Alignment>* alignments, int32_t maskLen, bool rebase = false, std::vector<uint16_t>* flags = 0) const {
    if (!targets_) throw std::runtime_error("BatchAligner::AlignWindows: no reference sequences");
    if (windows.size() != queries.size()) throw std::runtime_error("BatchAligner::AlignWindows: one window per query");
    const int32_t nq = (int32_t)queries.size();
    alignments->assign(queries.size(), Alignment());
    if (flags) flags->assign(queries.size(), 0);
    if (nq == 0) return;
    std::string text; std::vector<int64_t> off(1, 0);
    for (int32_t i = 0; i < nq; ++i) { text += queries[i]; off.push_back((int64_t)text.size()); }
    std::vector<int32_t> qidx((size_t)nq), tidx((size_t)nq), tlen((size_t)nq);
    std::vector<int64_t> tbeg((size_t)nq);
    for (int32_t i = 0; i < nq; ++i) {
      const Window& w = windows[(size_t)i];
      if (w.reference < 0 || w.reference >= n_targets_) throw std::runtime_error("BatchAligner::AlignWindows: no such reference sequence");
      qidx[(size_t)i] = i; tidx[(size_t)i] = w.reference; tbeg[(size_t)i] = w.begin; tlen[(size_t)i] = w.length;
    }
    ssw_gpu_seqs* Q = ssw_gpu_seqs_upload_ascii(ctx_, text.data(), off.data(), nq, table_.data());
    if (!Q) throw std::runtime_error(std::string("ssw_gpu_seqs_upload_ascii: ") + ssw_gpu_last_error(ctx_));
    ssw_gpu_params p; memset(&p, 0, sizeof p);
    p.mat = matrix_.data(); p.n = matrix_size_; p.gapO = gap_open_; p.gapE = gap_extend_;
    p.flag = (uint8_t)((filter.report_begin_position ? 0x08 : 0) | (filter.report_cigar ? 0x0f : 0));
    p.filters = filter.score_filter; p.filterd = filter.distance_filter; p.maskLen = std::max(maskLen, 15); p.score_size = 2;
    std::vector<ssw_gpu_result> res((size_t)nq);
    uint32_t* pool = 0; int64_t words = 0;
    const int rc = ssw_gpu_align_windows(ctx_, Q, targets_, qidx.data(), tidx.data(), tbeg.data(), tlen.data(), nq, &p, res.data(), &pool, &words);
    ssw_gpu_seqs_free(Q);
    if (rc != 0) { free(pool); throw std::runtime_error(std::string("ssw_gpu_align_windows: ") + (rc == SSW_GPU_BUSY ? ssw_gpu_strerror(rc) : ssw_gpu_last_error(ctx_))); }
    for (int32_t i = 0; i < nq; ++i) {
      const ssw_gpu_result& r = res[(size_t)i];
      Alignment& a = (*alignments)[(size_t)i];
      a.sw_score = r.score1; a.sw_score_next_best = r.score2; a.ref_begin = r.ref_begin1; a.ref_end = r.ref_end1;
      a.query_begin = r.read_begin1; a.query_end = r.read_end1; a.ref_end_next_best = r.ref_end2;
      if (flags) (*flags)[(size_t)i] = r.flag;
      const int8_t* ref = ref_codes_.data() + ref_off_[(size_t)tidx[(size_t)i]] + tbeg[(size_t)i];      // column 0 of the window
      Expand(a, r.cigarLen > 0 ? pool + r.cigar_off : 0, r.cigarLen, ref, text.data() + off[(size_t)i], (int)queries[(size_t)i].size());
      if (rebase) {      // a reference is below 2^31 residues and a position lies inside it: the sums fit
        const int32_t b = (int32_t)tbeg[(size_t)i];
        if (a.ref_begin >= 0) a.ref_begin += b;
        if (a.ref_end >= 0) a.ref_end += b;
        if (a.ref_end_next_best >= 0) a.ref_end_next_best += b;
      }
    }
    free(pool);
  }

  // The best candidate window of every read (ssw_gpu_align_windows_best): candidates[i] are the windows a mapper holds for queries[i]
  // (forward strand only here: a caller with both strands passes the reverse complement as a query of its own group, or uses the C ABI).
  // alignments[i] is what AlignWindows gives for queries[i] against the chosen window; (*best)[i].candidate is its index in
  // candidates[i] (-1: no candidate scored > 0 and >= min_score -- alignments[i] is then a default Alignment), runner_up / runner_up_score
  // the second of the ranking (sw_score descending, then index ascending; -1 / 0 when there is none), eligible how many qualified.
  // The forward fill runs once over all candidates, the selection on the device, begin positions and CIGARs for the winners only.
  struct BestWindow {
    int32_t candidate;
    int32_t runner_up;
    uint16_t runner_up_score;
    int32_t eligible;
    uint16_t flag;
  };
  void AlignWindowsBest(const std::vector<std::string>& queries, const std::vector<std::vector<Window> >& candidates, const Filter& filter,
                        std::vector<Alignment>* alignments, std::vector<BestWindow>* best, int32_t maskLen, int32_t min_score = 0,
                        bool rebase = false) const {
    if (!targets_) throw std::runtime_error("BatchAligner::AlignWindowsBest: no reference sequences");
    if (candidates.size() != queries.size()) throw std::runtime_error("BatchAligner::AlignWindowsBest: one candidate list per query");
    const int32_t nq = (int32_t)queries.size();
    alignments->assign(queries.size(), Alignment());
    BestWindow none; none.candidate = -1; none.runner_up = -1; none.runner_up_score = 0; none.eligible = 0; none.flag = 0;
    best->assign(queries.size(), none);
    if (nq == 0) return;
    std::string text; std::vector<int64_t> off(1, 0), cand_off(1, 0), tbeg;
    std::vector<int32_t> qidx, tidx, tlen;
    for (int32_t i = 0; i < nq; ++i) {
      text += queries[i]; off.push_back((int64_t)text.size());
      for (size_t k = 0; k < candidates[(size_t)i].size(); ++k) {
        const Window& w = candidates[(size_t)i][k];
        if (w.reference < 0 || w.reference >= n_targets_) throw std::runtime_error("BatchAligner::AlignWindowsBest: no such reference sequence");
        qidx.push_back(i); tidx.push_back(w.reference); tbeg.push_back(w.begin); tlen.push_back(w.length);
      }
      cand_off.push_back((int64_t)qidx.size());
    }
    ssw_gpu_seqs* Q = ssw_gpu_seqs_upload_ascii(ctx_, text.data(), off.data(), nq, table_.data());
    if (!Q) throw std::runtime_error(std::string("ssw_gpu_seqs_upload_ascii: ") + ssw_gpu_last_error(ctx_));
    ssw_gpu_params p; memset(&p, 0, sizeof p);
    p.mat = matrix_.data(); p.n = matrix_size_; p.gapO = gap_open_; p.gapE = gap_extend_;
    p.flag = (uint8_t)((filter.report_begin_position ? 0x08 : 0) | (filter.report_cigar ? 0x0f : 0));
    p.filters = filter.score_filter; p.filterd = filter.distance_filter; p.maskLen = std::max(maskLen, 15); p.score_size = 2;
    std::vector<ssw_gpu_result> res((size_t)nq);
    std::vector<ssw_gpu_best> sel((size_t)nq);
    uint32_t* pool = 0; int64_t words = 0;
    const int rc = ssw_gpu_align_windows_best(ctx_, Q, targets_, cand_off.data(), nq, qidx.data(), tidx.data(), tbeg.data(), tlen.data(), &p, min_score,
                                              sel.data(), res.data(), &pool, &words);
    ssw_gpu_seqs_free(Q);
    if (rc != 0) { free(pool); throw std::runtime_error(std::string("ssw_gpu_align_windows_best: ") + (rc == SSW_GPU_BUSY ? ssw_gpu_strerror(rc) : ssw_gpu_last_error(ctx_))); }
    for (int32_t i = 0; i < nq; ++i) {
      const ssw_gpu_best& s = sel[(size_t)i];
      BestWindow& b = (*best)[(size_t)i];
      b.candidate = s.best; b.runner_up = s.second; b.runner_up_score = s.second_score1; b.eligible = s.n_eligible;
      if (s.best < 0) continue;
      const ssw_gpu_result& r = res[(size_t)i];
      const size_t c = (size_t)(cand_off[(size_t)i] + s.best);
      Alignment& a = (*alignments)[(size_t)i];
      a.sw_score = r.score1; a.sw_score_next_best = r.score2; a.ref_begin = r.ref_begin1; a.ref_end = r.ref_end1;
      a.query_begin = r.read_begin1; a.query_end = r.read_end1; a.ref_end_next_best = r.ref_end2;
      b.flag = r.flag;
      Expand(a, r.cigarLen > 0 ? pool + r.cigar_off : 0, r.cigarLen, ref_codes_.data() + ref_off_[(size_t)tidx[c]] + tbeg[c], text.data() + off[(size_t)i],
             (int)queries[(size_t)i].size());
      if (rebase) {
        const int32_t sh = (int32_t)tbeg[c];
        if (a.ref_begin >= 0) a.ref_begin += sh;
        if (a.ref_end >= 0) a.ref_end += sh;
        if (a.ref_end_next_best >= 0) a.ref_end_next_best += sh;
      }
    }
    free(pool);
  }

  // The best k candidate windows of every read (ssw_gpu_align_windows_topk): AlignWindowsBest's candidate lists and ranking, k ranks per
  // read -- the primary alignment and its secondaries.  (*alignments)[i] holds one Alignment per REPORTED rank (at most k; fewer where
  // fewer candidates qualify or max_drop cuts the list: rank r >= 1 is reported only while its sw_score >= sw_score(rank 0) - max_drop,
  // max_drop < 0 for no cut), (*hits)[i][r] its candidate index and s_align flag, (*eligible)[i] how many candidates qualified whatever
  // k and max_drop are.  One forward fill over all candidates, the selection on the device, begin positions and CIGARs for the
  // reported ranks only.
  struct WindowHit {
    int32_t candidate;
    uint16_t flag;
  };
  void AlignWindowsTopK(const std::vector<std::string>& queries, const std::vector<std::vector<Window> >& candidates, const Filter& filter, int32_t k,
                        std::vector<std::vector<Alignment> >* alignments, std::vector<std::vector<WindowHit> >* hits, std::vector<int32_t>* eligible,
                        int32_t maskLen, int32_t min_score = 0, int32_t max_drop = -1, bool rebase = false) const {
    if (!targets_) throw std::runtime_error("BatchAligner::AlignWindowsTopK: no reference sequences");
    if (candidates.size() != queries.size()) throw std::runtime_error("BatchAligner::AlignWindowsTopK: one candidate list per query");
    if (k < 1 || k > SSW_GPU_GROUP_TOPK_MAX) throw std::runtime_error("BatchAligner::AlignWindowsTopK: k out of range");
    const int32_t nq = (int32_t)queries.size();
    alignments->assign(queries.size(), std::vector<Alignment>());
    hits->assign(queries.size(), std::vector<WindowHit>());
    eligible->assign(queries.size(), 0);
    if (nq == 0) return;
    std::string text; std::vector<int64_t> off(1, 0), cand_off(1, 0), tbeg;
    std::vector<int32_t> qidx, tidx, tlen;
    for (int32_t i = 0; i < nq; ++i) {
      text += queries[i]; off.push_back((int64_t)text.size());
      for (size_t c = 0; c < candidates[(size_t)i].size(); ++c) {
        const Window& w = candidates[(size_t)i][c];
        if (w.reference < 0 || w.reference >= n_targets_) throw std::runtime_error("BatchAligner::AlignWindowsTopK: no such reference sequence");
        qidx.push_back(i); tidx.push_back(w.reference); tbeg.push_back(w.begin); tlen.push_back(w.length);
      }
      cand_off.push_back((int64_t)qidx.size());
    }
    ssw_gpu_seqs* Q = ssw_gpu_seqs_upload_ascii(ctx_, text.data(), off.data(), nq, table_.data());
    if (!Q) throw std::runtime_error(std::string("ssw_gpu_seqs_upload_ascii: ") + ssw_gpu_last_error(ctx_));
    ssw_gpu_params p; memset(&p, 0, sizeof p);
    p.mat = matrix_.data(); p.n = matrix_size_; p.gapO = gap_open_; p.gapE = gap_extend_;
    p.flag = (uint8_t)((filter.report_begin_position ? 0x08 : 0) | (filter.report_cigar ? 0x0f : 0));
    p.filters = filter.score_filter; p.filterd = filter.distance_filter; p.maskLen = std::max(maskLen, 15); p.score_size = 2;
    std::vector<ssw_gpu_result> res((size_t)nq * (size_t)k);
    std::vector<int32_t> pos((size_t)nq * (size_t)k);
    uint32_t* pool = 0; int64_t words = 0;
    const int rc = ssw_gpu_align_windows_topk(ctx_, Q, targets_, cand_off.data(), nq, qidx.data(), tidx.data(), tbeg.data(), tlen.data(), &p, k, min_score,
                                              max_drop, pos.data(), eligible->data(), res.data(), &pool, &words);
    ssw_gpu_seqs_free(Q);
    if (rc != 0) { free(pool); throw std::runtime_error(std::string("ssw_gpu_align_windows_topk: ") + (rc == SSW_GPU_BUSY ? ssw_gpu_strerror(rc) : ssw_gpu_last_error(ctx_))); }
    for (int32_t i = 0; i < nq; ++i)
      for (int32_t r = 0; r < k; ++r) {
        const size_t o = (size_t)i * (size_t)k + (size_t)r;
        if (pos[o] < 0) break;
        const ssw_gpu_result& rec = res[o];
        const size_t c = (size_t)(cand_off[(size_t)i] + pos[o]);
        Alignment a;
        a.sw_score = rec.score1; a.sw_score_next_best = rec.score2; a.ref_begin = rec.ref_begin1; a.ref_end = rec.ref_end1;
        a.query_begin = rec.read_begin1; a.query_end = rec.read_end1; a.ref_end_next_best = rec.ref_end2;
        Expand(a, rec.cigarLen > 0 ? pool + rec.cigar_off : 0, rec.cigarLen, ref_codes_.data() + ref_off_[(size_t)tidx[c]] + tbeg[c], text.data() + off[(size_t)i],
               (int)queries[(size_t)i].size());
        if (rebase) {
          const int32_t sh = (int32_t)tbeg[c];
          if (a.ref_begin >= 0) a.ref_begin += sh;
          if (a.ref_end >= 0) a.ref_end += sh;
          if (a.ref_end_next_best >= 0) a.ref_end_next_best += sh;
        }
        WindowHit h; h.candidate = pos[o]; h.flag = rec.flag;
        (*alignments)[(size_t)i].push_back(a); (*hits)[(size_t)i].push_back(h);
      }
    free(pool);
  }

  // The best candidate pair of every read pair (ssw_gpu_align_windows_mates_lib): reads holds 2 * nfrag strings, mate 1 of fragment f at
  // 2 f and mate 2 at 2 f + 1, as the sequencer gives them; candidates[r] are the windows a mapper holds for reads[r], each on the strand
  // it says (reverse: the read's reverse complement is what is aligned -- the minus strand).  The reads are uploaded once and their
  // reverse complements built on the device (ssw_gpu_seqs_with_revcomp).  (*pairs)[f] is the selection of fragment f -- the candidate
  // indices in candidates[2 f] / candidates[2 f + 1] (-1: none), how many were eligible, the pair score S, the second combination's S, the
  // number of proper combinations and whether the chosen one is proper under `orientation` (SSW_GPU_MATES_FR / _RF / _FF) and
  // min_insert .. max_insert; (*alignments)[r] is what AlignWindows gives for the aligned sequence against the chosen window (a default
  // Alignment where nothing was chosen).  For a winner on the reverse strand the aligned sequence is the reverse complement of reads[r]:
  // query_begin / query_end and the '=' / 'X' runs of cigar_string refer to it (DNA tables: codes 0 .. 3 are complemented, every other
  // character is kept, as the device does).  rebase = true adds the chosen window's begin to the three reference positions.
  // insert_penalty (optional): the pair model's table (ssw_gpu_pair_model) -- max_insert - min_insert + 1 entries, entry i what a proper
  // combination of span min_insert + i pays where the flat rule has 0; another length throws.  nullptr: the flat rule, the same call as before.
  struct MateWindow {
    int32_t reference;
    int64_t begin;
    int32_t length;
    bool reverse;
  };
  struct MatePair {
    int32_t candidate1, candidate2;      // -1: none
    int32_t eligible1, eligible2;
    int32_t score, second_score;
    int32_t proper_count;
    bool proper;
    uint16_t flag1, flag2;               // s_align flag of the two alignments
  };
  void AlignWindowsMates(const std::vector<std::string>& reads, const std::vector<std::vector<MateWindow> >& candidates, const Filter& filter,
                         std::vector<Alignment>* alignments, std::vector<MatePair>* pairs, int32_t maskLen, int32_t min_insert, int32_t max_insert,
                         int32_t unpaired_penalty, int32_t min_score = 0, int32_t orientation = SSW_GPU_MATES_FR, bool rebase = false,
                         const std::vector<uint16_t>* insert_penalty = nullptr) const {
    if (!targets_) throw std::runtime_error("BatchAligner::AlignWindowsMates: no reference sequences");
    if (insert_penalty && (int64_t)insert_penalty->size() != (int64_t)max_insert - min_insert + 1)
      throw std::runtime_error("BatchAligner::AlignWindowsMates: insert_penalty must have max_insert - min_insert + 1 entries");
    if (reads.size() % 2 != 0) throw std::runtime_error("BatchAligner::AlignWindowsMates: two reads per fragment");
    if (candidates.size() != reads.size()) throw std::runtime_error("BatchAligner::AlignWindowsMates: one candidate list per read");
    const int32_t nr = (int32_t)reads.size(), nf = nr / 2;
    alignments->assign(reads.size(), Alignment());
    MatePair none; none.candidate1 = none.candidate2 = -1; none.eligible1 = none.eligible2 = 0; none.score = none.second_score = 0;
    none.proper_count = 0; none.proper = false; none.flag1 = none.flag2 = 0;
    pairs->assign((size_t)nf, none);
    if (nf == 0) return;
    std::string text; std::vector<int64_t> off(1, 0), cand_off(1, 0), tbeg;
    std::vector<int32_t> qidx, tidx, tlen;
    for (int32_t i = 0; i < nr; ++i) {
      text += reads[(size_t)i]; off.push_back((int64_t)text.size());
      for (size_t k = 0; k < candidates[(size_t)i].size(); ++k) {
        const MateWindow& w = candidates[(size_t)i][k];
        if (w.reference < 0 || w.reference >= n_targets_) throw std::runtime_error("BatchAligner::AlignWindowsMates: no such reference sequence");
        qidx.push_back(w.reverse ? nr + i : i); tidx.push_back(w.reference); tbeg.push_back(w.begin); tlen.push_back(w.length);
      }
      cand_off.push_back((int64_t)qidx.size());
    }
    ssw_gpu_seqs* F = ssw_gpu_seqs_upload_ascii(ctx_, text.data(), off.data(), nr, table_.data());
    if (!F) throw std::runtime_error(std::string("ssw_gpu_seqs_upload_ascii: ") + ssw_gpu_last_error(ctx_));
    ssw_gpu_seqs* Q = ssw_gpu_seqs_with_revcomp(ctx_, F);
    ssw_gpu_seqs_free(F);
    if (!Q) throw std::runtime_error(std::string("ssw_gpu_seqs_with_revcomp: ") + ssw_gpu_last_error(ctx_));
    ssw_gpu_params p; memset(&p, 0, sizeof p);
    p.mat = matrix_.data(); p.n = matrix_size_; p.gapO = gap_open_; p.gapE = gap_extend_;
    p.flag = (uint8_t)((filter.report_begin_position ? 0x08 : 0) | (filter.report_cigar ? 0x0f : 0));
    p.filters = filter.score_filter; p.filterd = filter.distance_filter; p.maskLen = std::max(maskLen, 15); p.score_size = 2;
    std::vector<ssw_gpu_result> res((size_t)nr);
    std::vector<ssw_gpu_mates> sel((size_t)nf);
    uint32_t* pool = 0; int64_t words = 0;
    int rc;
    if (insert_penalty) {
      ssw_gpu_pair_model model; memset(&model, 0, sizeof model);
      model.min_insert = min_insert; model.max_insert = max_insert; model.unpaired_penalty = unpaired_penalty; model.orientation = orientation;
      model.insert_penalty = insert_penalty->data();
      rc = ssw_gpu_align_windows_mates_model(ctx_, Q, targets_, cand_off.data(), nf, qidx.data(), tidx.data(), tbeg.data(), tlen.data(), nr, &p,
                                             min_score, &model, sel.data(), res.data(), &pool, &words);
    } else
      rc = ssw_gpu_align_windows_mates_lib(ctx_, Q, targets_, cand_off.data(), nf, qidx.data(), tidx.data(), tbeg.data(), tlen.data(), nr, &p,
                                           min_score, min_insert, max_insert, unpaired_penalty, orientation, sel.data(), res.data(), &pool, &words);
    ssw_gpu_seqs_free(Q);
    if (rc != 0) { free(pool); throw std::runtime_error(std::string("ssw_gpu_align_windows_mates: ") + (rc == SSW_GPU_BUSY ? ssw_gpu_strerror(rc) : ssw_gpu_last_error(ctx_))); }
    for (int32_t f = 0; f < nf; ++f) {
      const ssw_gpu_mates& s = sel[(size_t)f];
      MatePair& m = (*pairs)[(size_t)f];
      m.candidate1 = s.pos1; m.candidate2 = s.pos2; m.eligible1 = s.n_eligible1; m.eligible2 = s.n_eligible2;
      m.score = s.score; m.second_score = s.second_score; m.proper_count = s.n_proper; m.proper = s.proper != 0;
      for (int h = 0; h < 2; ++h) {
        const int32_t pos = h ? s.pos2 : s.pos1, i = 2 * f + h;
        if (pos < 0) continue;
        const ssw_gpu_result& r = res[(size_t)i];
        const size_t c = (size_t)(cand_off[(size_t)i] + pos);
        Alignment& a = (*alignments)[(size_t)i];
        a.sw_score = r.score1; a.sw_score_next_best = r.score2; a.ref_begin = r.ref_begin1; a.ref_end = r.ref_end1;
        a.query_begin = r.read_begin1; a.query_end = r.read_end1; a.ref_end_next_best = r.ref_end2;
        (h ? m.flag2 : m.flag1) = r.flag;
        const int qlen = (int)reads[(size_t)i].size();
        const std::string rcq = qidx[c] >= nr ? ReverseComplement(reads[(size_t)i]) : std::string();
        Expand(a, r.cigarLen > 0 ? pool + r.cigar_off : 0, r.cigarLen, ref_codes_.data() + ref_off_[(size_t)tidx[c]] + tbeg[c],
               qidx[c] >= nr ? rcq.data() : text.data() + off[(size_t)i], qlen);
        if (rebase) {
          const int32_t sh = (int32_t)tbeg[c];
          if (a.ref_begin >= 0) a.ref_begin += sh;
          if (a.ref_end >= 0) a.ref_end += sh;
          if (a.ref_end_next_best >= 0) a.ref_end_next_best += sh;
        }
      }
    }
    free(pool);
  }

  // A database search kept to its best hits (ssw_gpu_search_topk): (*hits)[i] holds, in rank order (sw_score descending, then reference
  // index ascending), up to k references of the set whose alignment with queries[i] scores > 0 and >= min_score -- each with the Alignment
  // and flag that AlignPairs gives for that pair.  maskLen < 15 is raised to 15 like there.
  struct TopKHit {
    int32_t target;
    Alignment alignment;
    uint16_t flag;
  };
  void SearchTopK(const std::vector<std::string>& queries, int32_t k, const Filter& filter, std::vector<std::vector<TopKHit> >* hits,
                  int32_t maskLen, int32_t min_score = 1) const {
    if (!targets_) throw std::runtime_error("BatchAligner::SearchTopK: no reference sequences");
    if (k < 1 || k > SSW_GPU_TOPK_MAX) throw std::runtime_error("BatchAligner::SearchTopK: k must be 1 .. SSW_GPU_TOPK_MAX");
    const int32_t nq = (int32_t)queries.size();
    hits->assign(queries.size(), std::vector<TopKHit>());
    if (nq == 0) return;
    std::string text; std::vector<int64_t> off(1, 0);
    for (int32_t i = 0; i < nq; ++i) { text += queries[i]; off.push_back((int64_t)text.size()); }
    ssw_gpu_seqs* Q = ssw_gpu_seqs_upload_ascii(ctx_, text.data(), off.data(), nq, table_.data());
    if (!Q) throw std::runtime_error(std::string("ssw_gpu_seqs_upload_ascii: ") + ssw_gpu_last_error(ctx_));
    ssw_gpu_params p; memset(&p, 0, sizeof p);
    p.mat = matrix_.data(); p.n = matrix_size_; p.gapO = gap_open_; p.gapE = gap_extend_;
    p.flag = (uint8_t)((filter.report_begin_position ? 0x08 : 0) | (filter.report_cigar ? 0x0f : 0));
    p.filters = filter.score_filter; p.filterd = filter.distance_filter; p.maskLen = std::max(maskLen, 15); p.score_size = 2;
    std::vector<int32_t> tidx((size_t)nq * (size_t)k);
    std::vector<ssw_gpu_result> res((size_t)nq * (size_t)k);
    uint32_t* pool = 0; int64_t words = 0;
    const int rc = ssw_gpu_search_topk(ctx_, Q, targets_, &p, k, min_score, 0, tidx.data(), res.data(), &pool, &words);
    ssw_gpu_seqs_free(Q);
    if (rc != 0) { free(pool); throw std::runtime_error(std::string("ssw_gpu_search_topk: ") + (rc == SSW_GPU_BUSY ? ssw_gpu_strerror(rc) : ssw_gpu_last_error(ctx_))); }
    for (int32_t i = 0; i < nq; ++i)
      for (int32_t r = 0; r < k; ++r) {
        const size_t s = (size_t)i * (size_t)k + (size_t)r;
        if (tidx[s] < 0) break;
        const ssw_gpu_result& g = res[s];
        TopKHit h;
        h.target = tidx[s]; h.flag = g.flag;
        Alignment& a = h.alignment;
        a.sw_score = g.score1; a.sw_score_next_best = g.score2; a.ref_begin = g.ref_begin1; a.ref_end = g.ref_end1;
        a.query_begin = g.read_begin1; a.query_end = g.read_end1; a.ref_end_next_best = g.ref_end2;
        Expand(a, g.cigarLen > 0 ? pool + g.cigar_off : 0, g.cigarLen, ref_codes_.data() + ref_off_[(size_t)tidx[s]], text.data() + off[(size_t)i],
               (int)queries[(size_t)i].size());
        (*hits)[(size_t)i].push_back(h);
      }
    free(pool);
  }

 private:
  // soft clips, '=' / 'X' runs and the mismatch count of one alignment: the outcome of the reference's ConvertAlignment +
  // CalculateNumberMismatch (ssw_cpp.cpp:52-89, 123-199).  Like there, the clips are written even when ssw_align returned no CIGAR
  // (CalculateNumberMismatch runs unconditionally: an alignment without a path ends up with just its soft clips).
  void Expand(Alignment& a, const uint32_t* cig, int32_t n_ops, const int8_t* ref, const char* query, int qlen) const {
    a.cigar.clear(); a.cigar_string.clear(); a.mismatches = 0;
    if (!cig) n_ops = 0;
    if (a.query_begin > 0) Push(a, (uint32_t)a.query_begin, 'S');
    const int8_t* rp = ref + (a.ref_begin > 0 ? a.ref_begin : 0);
    const char* qp = query + (a.query_begin > 0 ? a.query_begin : 0);
    uint32_t run = 0; char run_op = 0;
    for (int32_t k = 0; k < n_ops; ++k) {
      const char op = cigar_int_to_op(cig[k]);
      const uint32_t len = cigar_int_to_len(cig[k]);
      if (op == 'M') {
        for (uint32_t j = 0; j < len; ++j, ++rp, ++qp) {
          const char now = *rp != table_[(unsigned char)*qp & 127] ? 'X' : '=';
          if (now == 'X') ++a.mismatches;
          if (run > 0 && now != run_op) { Push(a, run, run_op); run = 0; }
          run_op = now; ++run;
        }
      } else if (op == 'I' || op == 'D') {
        if (run > 0) { Push(a, run, run_op); run = 0; }
        if (op == 'I') qp += len; else rp += len;
        a.mismatches += (int32_t)len;
        Push(a, len, op);
      }
    }
    if (run > 0) Push(a, run, run_op);
    const int end = qlen - a.query_end - 1;
    if (end > 0) Push(a, (uint32_t)end, 'S');
  }
  // what the device's reverse complement of a read looks like as text: reversed, a character of code c in 0 .. 3 replaced by one of
  // code 3 - c (A, C, G or T where the table knows them), every other character kept
  std::string ReverseComplement(const std::string& s) const {
    char comp[4];
    for (int c = 0; c < 4; ++c) {
      comp[c] = 0;
      for (const char* k = "ACGT"; *k && !comp[c]; ++k) if (table_[(unsigned char)*k] == 3 - c) comp[c] = *k;
      for (int k = 1; k < 128 && !comp[c]; ++k) if (table_[(size_t)k] == 3 - c) comp[c] = (char)k;
    }
    std::string out(s.rbegin(), s.rend());
    for (size_t i = 0; i < out.size(); ++i) {
      const int8_t c = table_[(unsigned char)out[i] & 127];
      if (c >= 0 && c < 4 && comp[c]) out[i] = comp[c];
    }
    return out;
  }
  static void Push(Alignment& a, uint32_t len, char op) {
    a.cigar.push_back(to_cigar_int(len, op));
    a.cigar_string += std::to_string(len);
    a.cigar_string += op;
  }
  void SetDnaScores(uint8_t match, uint8_t mismatch) {      // BuildSwScoreMatrix + the A/C/G/T/N table of ssw_cpp.cpp:13-50 (N scores -mismatch)
    matrix_size_ = 5;
    matrix_.assign(25, (int8_t)-(int)mismatch);
    for (int i = 0; i < 4; ++i) matrix_[(size_t)(i * 5 + i)] = (int8_t)match;
    table_.assign(128, 4);
    table_['A'] = table_['a'] = 0; table_['C'] = table_['c'] = 1; table_['G'] = table_['g'] = 2; table_['T'] = table_['t'] = 3;
  }
  BatchAligner(const BatchAligner&);             // one device context per object
  BatchAligner& operator=(const BatchAligner&);

  ssw_gpu_ctx* ctx_;
  ssw_gpu_seqs* targets_;
  int n_targets_;
  uint8_t gap_open_, gap_extend_;
  int matrix_size_;
  std::vector<int8_t> matrix_, table_, ref_codes_;
  std::vector<int64_t> ref_off_;
};

}  // namespace StripedSmithWaterman
#endif  // SSW_GPU_CPP_H
