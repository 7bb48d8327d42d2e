// decode_beam_rep.hip — beam_candidates_kernel under the repetition rules (DESIGN.md "Repetition rules"): the second
// instantiation of beam_candidates_body.inc. One workgroup per slot builds the ban and seen images (decode_rules.hpp:
// repetition_stage) from the hypothesis' own history in the beam records, in dynamic LDS, and proposes its M best ids of the edited
// row. A handle without rules never launches this: its candidates launch is decode_beam.hip's, with the arguments it always had.
#include "decode_beam_candidates.hpp"

namespace axw {
inline namespace AXW_NS {

__global__ __launch_bounds__(256) void beam_candidates_rep_kernel(BeamCandParams p, const RepRules* rules) {
  using namespace beam_cand;
#define AXW_BEAM_REP true
#define AXW_BEAM_RULES rules
#include "beam_candidates_body.inc"
#undef AXW_BEAM_REP
#undef AXW_BEAM_RULES
}

void launch_beam_candidates_rep(const BeamCandParams& p, const RepRules* rules, hipStream_t s) {
  if (p.stride % 4 != 0 || p.stride < p.n_vocab || p.ts_begin <= p.eot || p.ts_begin > p.n_vocab || p.n_cand_max < 1 || p.n_cand_max > kBeamMaxCand ||
      p.beam < 1 || !p.hist || !p.cand_id || !p.cand_logprob || !p.n_cand || !rules) {
    fprintf(stderr, "[ax_whisper] launch_beam_candidates_rep: unsupported row stride %ld / ids (eot %d, T %d, vocab %d) / %d candidates\n", p.stride,
            p.eot, p.ts_begin, p.n_vocab, p.n_cand_max);
    abort();
  }
  hipLaunchKernelGGL(beam_candidates_rep_kernel, dim3(p.n_slots), dim3(256), repetition_lds_bytes(p.eot), s, p, rules);
}

}  // inline namespace AXW_NS
}  // namespace axw
