/* pk2hip.h -- C ABI of libpk2hip.so, the MI355X (gfx950) implementation of the
 * PyKaldi2 sequence-training hot path.
 *
 * The reference (jzlianglu/pykaldi2) has no FFI of its own: its hot path is
 * Python calling torch.nn / PyKaldi / Horovod.  Each entry point below replaces
 * one of those third-party calls; the reference call site is cited.  The
 * boundary is plain C: raw device pointers, sizes, a hipStream_t passed as
 * void*.  No torch types.  All device memory (inputs, outputs, workspaces) is
 * allocated and owned by the caller; the library never allocates device memory
 * on the hot path (graph handles own their static arrays, created once).
 *
 * Every function returns 0 on success or a negative pk2_status; the message of
 * the last failure on the calling thread is at pk2_last_error().  Kernels are
 * enqueued on `stream`; nothing synchronises unless stated.
 */
#ifndef PK2HIP_H_
#define PK2HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  PK2_OK = 0,
  PK2_ERR_INVALID = -1,   /* bad argument */
  PK2_ERR_HIP = -2,       /* HIP runtime error (see pk2_last_error) */
  PK2_ERR_LIMIT = -3,     /* size exceeds a documented kernel limit */
  PK2_ERR_IO = -4,        /* file could not be read / bad format */
  PK2_ERR_NUMERIC = -5    /* a device computation failed (e.g. the decoder lost every token) */
} pk2_status;

const char* pk2_last_error(void);
int pk2_version(void);               /* ABI version, currently 1 */

/* ------------------------------------------------------------------ *
 * Denominator graph.  Replaces kaldi.chain.DenominatorGraph(den_fst, P)
 * (reference bin/train_chain.py:167,202).  Host arrays describe den.fst's
 * arcs: prob = exp(-weight), pdf = ilabel-1.  The library computes
 * initial_probs (100-iteration rule), builds its three arc orderings
 * (by destination / by source / by pdf) and uploads them once.
 * ------------------------------------------------------------------ */
typedef struct pk2_den_graph pk2_den_graph;

int pk2_den_graph_create(int32_t num_states, int32_t num_pdfs, int64_t num_arcs,
                         const int32_t* arc_src, const int32_t* arc_dst,
                         const int32_t* arc_pdf, const float* arc_prob,
                         int32_t start_state, pk2_den_graph** out);
/* Reads an OpenFst binary StdVectorFst (den.fst) -- StdVectorFst.read at
 * reference bin/train_chain.py:167. */
int pk2_den_graph_from_openfst(const char* path, int32_t num_pdfs, pk2_den_graph** out);
int pk2_den_graph_destroy(pk2_den_graph* g);
int pk2_den_graph_info(const pk2_den_graph* g, int32_t* num_states, int32_t* num_pdfs,
                       int64_t* num_arcs);
/* Copies initial_probs (num_states floats) to a host buffer. */
int pk2_den_graph_initial_probs(const pk2_den_graph* g, float* host_out);

/* Which kernels a denominator call on num_seqs sequences takes on the current device: 0 = per-arc-pdf kernels,
 * 1 = state-x kernels, one launch per frame, 2 = state-x, persistent recursion kernel (one launch per call).  Reporting
 * only; the choice is the library's (reference: kaldi.chain.DenominatorComputation behind ops/ops.py:265). */
int32_t pk2_den_graph_path(const pk2_den_graph* g, int32_t num_seqs);
/* The form of the persistent recursion kernel behind path 2: 2 = chunked LDS table whose copy overlaps the arcs, two
 * resident passes and streamed overflow (any graph with < 65536 states); 0 = none (paths 0 / 1).  1 was the first such
 * kernel (everything resident) and is no longer returned.  PK2_DEN_PERSIST = 0 | 2 forces one; 1 makes the calls fail
 * with PK2_ERR_INVALID. */
int32_t pk2_den_graph_persist_form(const pk2_den_graph* g, int32_t num_seqs);
/* The route of a call on num_seqs sequences of at most max_frames frames, as the library decides it once per call
 * ("How a call is routed"): out = {family (0 = per-arc-pdf, 1 = state-x), persistent form, sequences per
 * group, buffers filled with zeros first, x gathered by pdf, launches in front of the recursions merged, launches behind
 * them mergeable, occupancy kernel (1 = row staged in LDS, 0 = gather)}.  Reporting only. */
int pk2_den_graph_plan(const pk2_den_graph* g, int32_t num_seqs, int32_t max_frames, int32_t out[8]);

/* ------------------------------------------------------------------ *
 * LF-MMI objective and derivative for a minibatch of N sequences.
 * Replaces kaldi.chain.compute_chain_objf_and_deriv (reference ops/ops.py:265)
 * plus the wrapper's own grad += xent_regularize * grad_xent (ops/ops.py:267),
 * without the host round trips of ops/ops.py:255,261,269-271.
 *
 * logits: device f32; sequence n, frame t, pdf p at
 *         logits[n*seq_stride + t*frame_stride + p]   (frame_stride >= P).
 * lengths: host int32[N], frames_per_sequence of each supervision.
 * grad:   device f32, same addressing as logits (grad_seq_stride/frame_stride);
 *         receives d objf / d logits for t < lengths[n] and 0 for the padding
 *         frames lengths[n] <= t < max_frames.
 * Numerator supervisions (Kaldi chain::Supervision FSTs: acyclic, one frame
 * per arc, label = pdf) are concatenated over the batch, on the device:
 *   num_arc_src/dst/pdf int32[total_arcs], num_arc_weight f32 (-log prob),
 *   arcs of one sequence sorted by the frame of their source state;
 *   num_frame_off int32[sum(lengths)+N]: for sequence n (base = sum_{m<n}
 *   (lengths[m]+1)) entry base+t is the first arc (global index) leaving frame
 *   t, entry base+lengths[n] is one past the last;
 *   num_state_off int32[N+1] gives each sequence's state-id base (arc src/dst
 *   are local to the sequence); state 0 is initial;
 *   num_final_state int32[total_finals], num_final_weight f32,
 *   num_final_off int32[N+1].
 * out (device f32[3*N]): objf[n] = weight*(log p_num - log p_den),
 *   num_logprob[n], den_logprob[n].  Kaldi's guard is mirrored: if a value is
 *   not finite or the alpha-beta check fails, objf[n] = -10*weight*lengths[n]
 *   and that sequence's gradient is zero.
 * workspace: device, at least pk2_chain_workspace_bytes() bytes.
 * ------------------------------------------------------------------ */
typedef struct {
  const int32_t* arc_src;
  const int32_t* arc_dst;
  const int32_t* arc_pdf;
  const float* arc_weight;
  const int32_t* frame_off;
  const int32_t* state_off;     /* host pointer, int32[N+1] */
  const int32_t* final_state;
  const float* final_weight;
  const int32_t* final_off;     /* host pointer, int32[N+1] */
  int64_t total_arcs;
  int64_t max_seq_arcs;         /* arcs of the largest single sequence (0 = unknown: total_arcs is the bound).  Decides
                                 * whether a sequence's frame table and arcs fit the LDS of its workgroup (the staged
                                 * forward-backward, which also rides inside the persistent denominator launch). */
} pk2_num_batch;

size_t pk2_chain_workspace_bytes(const pk2_den_graph* g, int32_t num_seqs, int32_t max_frames,
                                 int64_t num_total_states);

int pk2_chain_objf_and_deriv(const pk2_den_graph* g, const float* logits, int64_t seq_stride,
                             int64_t frame_stride, const int32_t* lengths, int32_t num_seqs,
                             const pk2_num_batch* num, float leaky_hmm_coefficient,
                             float xent_regularize, float l2_regularize, float weight,
                             float* grad, int64_t grad_seq_stride, int64_t grad_frame_stride,
                             float* out, void* workspace, size_t workspace_bytes, void* stream);

/* The same computation in the convention of the reference's autograd operator (ops/ops.py:243-280: forward returns the
 * objective, backward returns MINUS its derivative whatever grad_out is): the gradient written is
 * grad_scale * d objf / d logits (grad_scale = -1 for the operator) and *objf_sum (device f32, optional) receives
 * sum_n objf[n] -- so that the operator needs no elementwise or reduction kernel of its own around the call. */
int pk2_chain_objf_and_deriv_op(const pk2_den_graph* g, const float* logits, int64_t seq_stride,
                                int64_t frame_stride, const int32_t* lengths, int32_t num_seqs,
                                const pk2_num_batch* num, float leaky_hmm_coefficient,
                                float xent_regularize, float l2_regularize, float weight,
                                float* grad, int64_t grad_seq_stride, int64_t grad_frame_stride,
                                float* out, void* workspace, size_t workspace_bytes, float grad_scale,
                                float* objf_sum, void* stream);

/* Denominator only (log p_den and its occupancies); used by tests/profiling.
 * den_logprob: device f32[N]; gamma: device, logits addressing, receives
 * d log p_den / d logits (posteriors, rows sum to 1). */
int pk2_chain_den_fwd_bwd(const pk2_den_graph* g, const float* logits, int64_t seq_stride,
                          int64_t frame_stride, const int32_t* lengths, int32_t num_seqs,
                          float leaky_hmm_coefficient, float* den_logprob, float* gamma,
                          int64_t gamma_seq_stride, int64_t gamma_frame_stride, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Test hook: the objective / guard rule of pk2_chain_objf_and_deriv (Kaldi ComputeChainObjfAndDeriv: objf finite and
 * |alpha-beta product - 1| <= 2.0, else objf = -10 * weight * frames and a zero derivative) applied to given device arrays
 * of N per-sequence quantities.  out: device f32[3N] = {objf, num_lp, den_lp}; flags: device i32[N]. */
int pk2_chain_debug_flags(const float* num_lp, const float* den_lp, const float* alpha_beta_product,
                          const int32_t* lengths, int32_t N, float weight, float* out, int32_t* flags, void* stream);

/* Reporting hook: where the forward-backward of the supervised numerator ran in the last pk2_chain_objf_and_deriv[_op] call
 * of the process, as the host code decided it: out = {staged (frame table and arcs copied into LDS),
 * carrier, threads of the routine (256, 128 or 64), its LDS bytes}; carrier: 0 = none yet (or the call failed first),
 * 1 = stand-alone launch, 2 = inside the occupancy launch, LDS-row variant, 3 = the same, gather variant, 4 = tasks of the
 * persistent denominator launch, 5 = stand-alone on the internal side stream.  It changes no decision and launches nothing. */
int pk2_chain_debug_num_route(int32_t out[4]);

/* ------------------------------------------------------------------ *
 * Chain supervision of one utterance from its alignment (host-side integer work, no device memory).
 * Replaces, for bin/train_chain.py:262-272 of the reference,
 *   aligner.to_phone_alignment(trans_ids)                       (Kaldi SplitToPhones),
 *   kaldi.chain.alignment_to_proto_supervision(opts, phones, durations),
 *   kaldi.chain.proto_supervision_to_supervision(tree, trans_model, proto, convert_to_pdfs=True).
 * Kaldi composes the phone sequence with the context and H transducers, adds self-loops (reordered) and
 * composes with a time-enforcing FST; the frame-synchronous acceptor those operations define is built
 * here directly: state = (frames consumed, phone instance, HMM state of the last frame), see
 * csrc/chain_sup.hip.  Arc weights are 0 (Kaldi builds H with transition_scale = 0 and adds the self-loops
 * with self_loop_scale = 0).
 * ------------------------------------------------------------------ */
/* Splits a transition-id alignment into phones.  Tables are indexed by transition-id (1-based, entry 0
 * unused): tid_tstate = transition-state, tid_phone, tid_flags bit 0 = self-loop, bit 1 = transition to the
 * final HMM state.  phones / durations: capacity T.  Returns PK2_ERR_INVALID for a transition-id out of
 * range; *ok = 0 when the alignment is not a complete sequence of phones (Kaldi's SplitToPhones returns
 * false: the pieces are still produced). */
int pk2_split_to_phones(const int32_t* tid_tstate, const int32_t* tid_phone, const uint8_t* tid_flags,
                        int32_t num_tids, const int32_t* alignment, int32_t T, int32_t* phones,
                        int32_t* durations, int32_t* num_phones, int32_t* ok);

/* HMM topologies + context-dependency tree of the chain model (0.trans_mdl and tree of the reference's
 * -chain_dir).
 * Topology: phone2entry[max_phone+1] (-1 = phone without topology); entry e owns the HMM states
 *   entry_state_off[e] .. entry_state_off[e+1]; per state forward / self-loop pdf-class (-1 = non-emitting
 *   final state) and its transitions trans_dst[state_trans_off[s] .. state_trans_off[s+1]) given as HMM
 *   state indices inside the entry.
 * Tuples (optional, num_tuples = 0 skips the check): {phone, hmm_state, forward_pdf, self_loop_pdf} rows of
 *   the transition model; a (phone, state, pdfs) combination the tree produces that is not among them is an
 *   error, as in TransitionModel::TupleToTransitionState.
 * Tree: context width N, central position P, and the EventMap flattened to nodes
 *   kind 0 (constant): a = pdf-id;
 *   kind 1 (table):    key, children = pool[a .. a+b) (node index, -1 = null);
 *   kind 2 (split):    key, yes-set = pool[a .. a+b) sorted ascending, yes child = pool[a+b], no child = pool[a+b+1];
 *   keys: -1 = pdf-class, 0..N-1 = phone at that window position.  Node 0 is the root. */
typedef struct pk2_sup_model pk2_sup_model;
pk2_sup_model* pk2_sup_model_create(int32_t max_phone, const int32_t* phone2entry, int32_t num_entries,
                                    const int32_t* entry_state_off, const int32_t* state_fwd_class,
                                    const int32_t* state_loop_class, const int32_t* state_trans_off,
                                    const int32_t* trans_dst, int32_t num_tuples, const int32_t* tuples,
                                    int32_t context_width, int32_t central_position, int32_t num_nodes,
                                    const int32_t* node_kind, const int32_t* node_key, const int32_t* node_a,
                                    const int32_t* node_b, int32_t pool_size, const int32_t* pool);
void pk2_sup_model_destroy(pk2_sup_model* m);
/* ContextDependency::Compute: window[N] phones (0 = beyond the utterance) -> pdf-id; PK2_ERR_INVALID when the
 * tree has no answer. */
int pk2_sup_model_pdf(const pk2_sup_model* m, const int32_t* window, int32_t pdf_class, int32_t* pdf);

/* AlignmentToProtoSupervision + ProtoSupervisionToSupervision (convert_to_pdfs = true).
 * frames = ceil(sum(durations) / subsampling); phone i spanning frames [b, e) of the alignment may be emitted
 * on subsampled frames ceil(max(0, b - left_tolerance) / f) .. ceil(min(T, e + right_tolerance) / f) - 1;
 * the per-frame test is on the phone identity (TimeEnforcerFst).  Returns null (pk2_last_error) when no
 * path satisfies the constraints or a phone has no topology / tree answer / tuple. */
typedef struct pk2_supervision pk2_supervision;
pk2_supervision* pk2_supervision_create(const pk2_sup_model* m, const int32_t* phones,
                                        const int32_t* durations, int32_t num_phones, int32_t subsampling,
                                        int32_t left_tolerance, int32_t right_tolerance);
void pk2_supervision_destroy(pk2_supervision* s);
void pk2_supervision_sizes(const pk2_supervision* s, int32_t* frames, int32_t* num_states, int32_t* num_arcs,
                           int32_t* num_final, int32_t* num_allowed);
/* Arrays in the layout of pk2_num_batch for one sequence: arcs sorted by the frame of their source state,
 * frame_off[frames+1], states numbered in time order (state 0 initial), state_time[num_states].
 * allowed_off[frames+1] / allowed_phones: the ProtoSupervision's sorted allowed-phone sets.  Null pointers
 * are skipped. */
int pk2_supervision_copy(const pk2_supervision* s, int32_t* arc_src, int32_t* arc_dst, int32_t* arc_pdf,
                         float* arc_weight, int32_t* frame_off, int32_t* state_time, int32_t* final_state,
                         float* final_weight, int32_t* allowed_off, int32_t* allowed_phones);

/* ------------------------------------------------------------------ *
 * Forced alignment (kaldi.alignment.MappedAligner.align, reference bin/train_se2.py:192-199,263): training graphs
 * compiled on the host (csrc/align_graph.hip: transcript x L.fst x tree x H with reordered self-loops, built directly),
 * one Viterbi launch for a minibatch on the device (csrc/align_viterbi.hip).
 * ------------------------------------------------------------------ */
/* L.fst: input labels are phones, output labels words; input labels listed in `disambig` count as epsilon. */
typedef struct pk2_lexicon pk2_lexicon;
pk2_lexicon* pk2_lexicon_create(int32_t num_states, int32_t start, int64_t num_arcs, const int32_t* src, const int32_t* dst,
                                const int32_t* ilabel, const int32_t* olabel, const float* weight, const float* final_cost,
                                const int32_t* disambig, int32_t num_disambig);
pk2_lexicon* pk2_lexicon_from_openfst(const char* path, const int32_t* disambig, int32_t num_disambig);
void pk2_lexicon_destroy(pk2_lexicon* lexicon);
/* The tree and topologies of `m` (copied), the transition model's tuples in its order (they number the transition-ids),
 * log_probs[num_tids + 1] (entry 0 unused) and the two graph scales.  Fails for a context window other than N = 1,
 * N = 2 (P = 0 or 1), N = 3 (P = 1). */
typedef struct pk2_align_model pk2_align_model;
pk2_align_model* pk2_align_model_create(const pk2_sup_model* m, int32_t num_tuples, const int32_t* tuples, int32_t num_tids,
                                        const double* log_probs, double transition_scale, double self_loop_scale);
void pk2_align_model_destroy(pk2_align_model* model);
/* Training graphs of a batch: transcript n = words[word_off[n] .. word_off[n+1]), frames[n] frames.  Per utterance a
 * status: 0 = compiled, 2 = no path of that many frames, 3 = error (unknown word, no lexicon path, epsilon cycle, a
 * phone the model lacks; pk2_align_graphs_error has the reason).  Null only for bad arguments. */
typedef struct pk2_align_graphs pk2_align_graphs;
pk2_align_graphs* pk2_align_compile(const pk2_align_model* model, const pk2_lexicon* lexicon, int32_t num_utts,
                                    const int32_t* word_off, const int32_t* words, const int32_t* frames);
void pk2_align_graphs_destroy(pk2_align_graphs* graphs);
int pk2_align_graphs_info(const pk2_align_graphs* graphs, int32_t utt, int32_t* status, int32_t* num_states, int32_t* num_arcs);
const char* pk2_align_graphs_error(const pk2_align_graphs* graphs, int32_t utt);
/* One graph: in-arcs of state s are in_off[s] .. in_off[s+1], ordered by (source, transition-id); arc_src = -1 marks an
 * arc from the start state.  final_cost = +inf for non-final states.  Null pointers are skipped. */
int pk2_align_graphs_copy(const pk2_align_graphs* graphs, int32_t utt, int32_t* in_off, int32_t* arc_src, int32_t* arc_tid,
                          int32_t* arc_pdf, float* arc_weight, float* final_cost);
/* The batch as one int32 buffer (copy it to the device in one transfer) and the workspace pk2_align_viterbi needs. */
int64_t pk2_align_graphs_packed_words(const pk2_align_graphs* graphs);
int pk2_align_graphs_pack(const pk2_align_graphs* graphs, int32_t* out);
size_t pk2_align_workspace_bytes(const pk2_align_graphs* graphs);
/* 1 when the next pk2_align_viterbi keeps costs and graph in LDS (the graph fits and PK2_ALIGN_LDS is not 0). */
int pk2_align_use_lds(const pk2_align_graphs* graphs);
/* Viterbi of every utterance, one workgroup each, on `stream`.  packed_dev: the pk2_align_graphs_pack buffer on the device.
 * loglikes: device f32, frame t of utterance n at loglikes[n * seq_stride + t * frame_stride], num_pdfs columns, already
 * prior-subtracted; only frames < frames[n] are read.  Outputs (device): alignment i32[N][Tmax] (transition-ids, 0 past
 * the end and for failed utterances), costs f32[N][3] = {total, graph, acoustic} (+inf when failed), status i32[N] =
 * 0 ok, 1 no final state within the beam, 2 / 3 as compiled.  The arithmetic is specified in csrc/align_viterbi.hip. */
int pk2_align_viterbi(const pk2_align_graphs* graphs, const int32_t* packed_dev, const float* loglikes, int64_t seq_stride,
                      int64_t frame_stride, int32_t num_pdfs, int32_t Tmax, float acoustic_scale, float beam,
                      int32_t* alignment, float* costs, int32_t* status, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ------------------------------------------------------------------ *
 * Alignment-free LF-MMI ("flat-start" / e2e chain): the numerator is the full sum over every path of exactly frames[n]
 * frames through the training graph of utterance n (pk2_align_compile; csrc/chain_num_graph.hip):
 *   alpha_0(d) = sum_{a: dst=d, src=-1} exp(-w_a + x[0, pdf_a]),  alpha_t(d) = sum_{a: dst=d, src>=0} alpha_{t-1}(src_a) exp(-w_a + x[t, pdf_a]),
 *   log p_num  = log sum_s alpha_{T-1}(s) exp(-final[s]),         posterior[t, p] = d log p_num / d x[t, p].
 * No beam, logits unscaled.  An utterance without a graph (status 2: no path of that length; 3: not compiled) takes no part:
 * log p_num = 0 and its rows are not touched.
 * ------------------------------------------------------------------ */
size_t pk2_num_graph_workspace_bytes(const pk2_align_graphs* graphs);
/* 1 when the next call keeps the working vectors and the arcs in LDS (they fit and PK2_NUM_GRAPH_LDS is not 0). */
int pk2_num_graph_use_lds(const pk2_align_graphs* graphs);
/* The numerator alone (tests, tools).  logits / grad: device f32 addressed as in pk2_chain_objf_and_deriv, num_pdfs columns;
 * scale * posterior is ADDED into grad rows t < frames[n].  logprob f32[N], status i32[N] (0, or 2 / 3 as compiled): device.
 * workspace: device, 256-byte aligned, pk2_num_graph_workspace_bytes().  The result is bit-reproducible. */
int pk2_num_graph_fwd_bwd(const pk2_align_graphs* graphs, const int32_t* packed_dev, const float* logits, int64_t seq_stride,
                          int64_t frame_stride, int32_t num_pdfs, int32_t Tmax, float scale, float* grad, int64_t grad_seq_stride,
                          int64_t grad_frame_stride, float* logprob, int32_t* status, void* workspace, size_t workspace_bytes,
                          void* stream);
/* pk2_chain_objf_and_deriv[_op] with the graphs in place of pk2_num_batch: lengths are the graphs' frame counts, the
 * denominator, the regularisers and the non-finite-objective rule are those of the alignment-based entry.  An utterance
 * without a graph is left out of the denominator too: its three outputs and its gradient rows are 0.  Rows t < max_n frames[n]
 * of grad are written.  workspace: device, 256-byte aligned, pk2_chain_graph_workspace_bytes(). */
size_t pk2_chain_graph_workspace_bytes(const pk2_den_graph* g, const pk2_align_graphs* graphs);
int pk2_chain_objf_and_deriv_graph(const pk2_den_graph* g, const float* logits, int64_t seq_stride, int64_t frame_stride,
                                   const pk2_align_graphs* graphs, const int32_t* packed_dev, float leaky_hmm_coefficient,
                                   float xent_regularize, float l2_regularize, float weight, float* grad,
                                   int64_t grad_seq_stride, int64_t grad_frame_stride, float* out, void* workspace,
                                   size_t workspace_bytes, void* stream);
int pk2_chain_objf_and_deriv_graph_op(const pk2_den_graph* g, const float* logits, int64_t seq_stride, int64_t frame_stride,
                                      const pk2_align_graphs* graphs, const int32_t* packed_dev, float leaky_hmm_coefficient,
                                      float xent_regularize, float l2_regularize, float weight, float* grad,
                                      int64_t grad_seq_stride, int64_t grad_frame_stride, float* out, void* workspace,
                                      size_t workspace_bytes, float grad_scale, float* objf_sum, void* stream);

/* ------------------------------------------------------------------ *
 * Reverberation + additive noise of one utterance (single channel), device arrays throughout.
 * Replaces the numpy arithmetic of the reference's dynamic data simulation: Distorter.apply_rir /
 * Distorter.add_noise (reference simulation/_distorter.py:86-154) as _Simulator.simulate uses them for one
 * speech source (simulation/simulation.py:55-178, called from data/sr_dataset.py:321-345).  The random draws
 * (SNR, noise position) are made by the host and passed in.
 * ------------------------------------------------------------------ */
/* out[i] = (rir * wav)[delay - 1 + i], i in [0, n): apply_rir with sync = True (:147-148); delay = argmax(rir)
 * (delay = 0 keeps the direct path at sample 0).  out must not alias wav. */
int pk2_sim_apply_rir(const float* wav, int64_t n, const float* rir, int32_t k, int32_t delay, float* out,
                      void* stream);
/* pk2_sim_apply_rir with delay = *delay read from device memory (int32, clamped to [0, k)): reverberation by a RIR made
 * on the device (pk2_rirgen writes each row's argmax) without reading the delay back to the host. */
int pk2_sim_apply_rir_dev(const float* wav, int64_t n, const float* rir, int32_t k, const int32_t* delay, float* out,
                          void* stream);
/* stats (device f64[2], zeroed by the caller): stats[0] += sum x^2, stats[1] = max(stats[1], max |x|). */
int pk2_sim_power(const float* x, int64_t n, double* stats, void* stream);
/* mixed[i] += scale * noise_placed[i], scale = sqrt(Px / Pn * 10^(-snr_db / 10)) with Px = sig_stats[0] / n and
 * Pn = noise_stats[0] / m (_comp_noise_scale_given_snr :28-32); 'sample_noise' placement (:36-58): a noise not
 * longer than the signal sits at [start, start + m), a longer one is cropped from `start`. */
int pk2_sim_add_noise(float* mixed, int64_t n, const float* noise, int64_t m, int64_t start, float snr_db,
                      const double* sig_stats, const double* noise_stats, void* stream);
/* x *= 0.5 / stats[1]  (gain normalisation, simulation/simulation.py:170-172). */
int pk2_sim_gain_norm(float* x, int64_t n, const double* stats, void* stream);

/* ------------------------------------------------------------------ *
 * Multi-channel, multi-source simulation (reference simulation/simulation.py `_Simulator.simulate`, _mixer.py
 * `Mixer`, _distorter.py with C > 1).  Device layout: channel-major, a signal is a contiguous f32 (C, T) array and
 * a RIR is (C, k) (the reference uses (T, C)).  The job / segment / source tables are HOST arrays of at most
 * PK2_SIM_MAX_SEGS entries, passed to the kernel by value; every pointer inside them is device memory.
 * ------------------------------------------------------------------ */
#define PK2_SIM_MAX_SEGS 16
typedef struct {
  const float* wav;          /* (n) dry source */
  const float* rir;          /* (C, k) */
  float* out;                /* (C, n) reverberant source, pk2_sim_apply_rir per row */
  float* early;              /* (C, n) early reverberation, or NULL */
  const int32_t* delay_dev;  /* device int32 (clamped to [0, k)), or NULL: `delay` below */
  int64_t n;
  int32_t k;
  int32_t delay;             /* argmax of the source's channel-0 RIR: every row of the source uses it */
} pk2_sim_rir_job;
/* One launch for all (source, channel) rows.  early = the same convolution over the taps [0, min(k, early_taps + delay))
 * (early_taps = int(0.04 fs)), bit-equal to out computed with the RIR cut there. */
int pk2_sim_apply_rir_mc(const pk2_sim_rir_job* jobs, int32_t njobs, int32_t channels, int32_t early_taps, void* stream);

typedef struct {
  float* x;
  int64_t count;
} pk2_sim_seg;
/* stats (device f64 (nseg, 2), zeroed by the caller): pk2_sim_power of every segment in one launch. */
int pk2_sim_power_seg(const pk2_sim_seg* segs, int32_t nseg, double* stats, void* stream);
/* every segment *= 0.5 / stats[1]; gain (device f64[1], or NULL) receives that factor. */
int pk2_sim_gain_norm_seg(const pk2_sim_seg* segs, int32_t nseg, const double* stats, double* gain, void* stream);

typedef struct {
  const float* sig;    /* (C, n) reverberant source */
  const float* sig2;   /* (C, n) second signal (early reverberation) or NULL */
  float* pos;          /* (C, T) out or NULL: sig placed at `start`, unscaled */
  float* pos2;         /* (C, T) out or NULL: scale * sig2 placed at `start` */
  int64_t n;
  int64_t start;
  double spr_db;       /* 0 for source 0 */
} pk2_sim_mix_src;
/* Mixer.mix_signals: scale[i] = sqrt(P_0 / P_i * 10^(spr_i / 10)), P_i = stats[i][0] / (C n_i) (pk2_sim_power_seg);
 * mixed (C, T) = sum_i scale[i] * sig_i placed at start_i (sum in source order); scales: device f64[nsrc] out. */
int pk2_sim_mix(const pk2_sim_mix_src* srcs, int32_t nsrc, int32_t channels, int64_t T, const double* stats, float* mixed,
                double* scales, void* stream);
/* pk2_sim_add_noise over C rows, powers = means over all channels.  repeat = 0: 'sample_noise' placement; repeat = 1:
 * 'repeat_noise' (_NoiseSampler.repeat_noise): the noise tiled ceil(n / m) times when shorter, read at (start + i) mod m;
 * start in [0, tiled length - n]. */
int pk2_sim_add_noise_mc(float* mixed, int64_t n, const float* noise, int64_t m, int32_t channels, int64_t start,
                         float snr_db, int32_t repeat, const double* sig_stats, const double* noise_stats, void* stream);

/* ------------------------------------------------------------------ *
 * Sampling-rate conversion of a ragged minibatch: Kaldi's LinearResample / ResampleWaveform (polyphase windowed sinc),
 * the arithmetic of speed perturbation (resample rate_in = round(fs * factor) -> rate_out = fs) with the volume gain
 * folded in.  No counterpart in the reference; the contract is restated in DESIGN.md 7.7.
 *   g = gcd(rate_in, rate_out), iu = rate_in / g, ou = rate_out / g, cutoff = 0.99 * 0.5 * min(rate_in, rate_out),
 *   ww = num_zeros / (2 cutoff); phase p in [0, ou): t = p / rate_out, first[p] = ceil((t - ww) rate_in),
 *   last[p] = floor((t + ww) rate_in), taps[p] = last - first + 1,
 *   w[p][j] = f(dt) h(dt) / rate_in at dt = (first[p] + j) / rate_in - t   (Hann-windowed sinc, computed in double and
 *   rounded to float32 once);  y[u ou + p] = gain * sum_j w[p][j] x[first[p] + u iu + j], x = 0 outside [0, n_in).
 * rate_in == rate_out is the plan iu = ou = 1, first = 0, one weight 1: a copy (times the gain).
 * A plan is a host object: creating, inspecting and exporting it needs no GPU.  Its tables go to a device on the first
 * launch there (one allocation and one blocking copy per plan and device) and are freed by pk2_resample_plan_destroy.
 * ------------------------------------------------------------------ */
typedef struct pk2_resample_plan pk2_resample_plan;
/* cutoff_hz = 0: the default above; otherwise 0 < cutoff_hz <= 0.5 min(rate_in, rate_out).  num_zeros >= 1.
 * PK2_ERR_LIMIT when even the smallest output tile would read more input than the kernel stages (rate_in / rate_out
 * beyond about 20) or a phase has more than PK2_RESAMPLE_MAX_TAPS taps. */
#define PK2_RESAMPLE_MAX_TAPS 1024
int pk2_resample_plan_create(int32_t rate_in, int32_t rate_out, double cutoff_hz, int32_t num_zeros,
                             pk2_resample_plan** plan);
int pk2_resample_plan_destroy(pk2_resample_plan* plan);
/* tile: consecutive outputs one workgroup owns; table_bytes: what a device holds for the plan.  Any pointer may be NULL. */
int pk2_resample_plan_info(const pk2_resample_plan* plan, int32_t* iu, int32_t* ou, int32_t* max_taps, int32_t* tile,
                           int64_t* table_bytes);
/* Host arrays: first (ou) int32, taps (ou) int32, weights (ou, max_taps) float32, zero beyond taps[p]. */
int pk2_resample_plan_export(const pk2_resample_plan* plan, int32_t* first, int32_t* taps, float* weights);
/* ceil(n_in * rate_out / rate_in) (Kaldi's flushed length); -1 on a bad argument. */
int64_t pk2_resample_num_output(const pk2_resample_plan* plan, int64_t n_in);

/* The job table is a HOST array of at most PK2_RESAMPLE_MAX_JOBS entries that travels as a kernel argument; `in` / `out`
 * are device memory and must not overlap.  1 <= n_out <= pk2_resample_num_output(plan, n_in). */
#define PK2_RESAMPLE_MAX_JOBS 32
typedef struct {
  const pk2_resample_plan* plan;
  const float* in;
  int64_t n_in;
  float* out;
  int64_t n_out;
  float gain;     /* multiplies the finished float32 sum once */
} pk2_resample_job;
/* One launch for all jobs: a workgroup owns one tile of consecutive outputs of one job, stages the input span the tile
 * reads in LDS (zeros outside [0, n_in)) and the plan's weight table too when ou * max_taps <= 4096 and ou <= 512 (else it
 * reads the table from memory).  float32 accumulation in tap order, one writer per output, no atomics: a job's result is
 * bit-reproducible and does not depend on the other jobs. */
int pk2_resample_batch(const pk2_resample_job* jobs, int32_t njobs, void* stream);
/* Where the jobs of the most recent pk2_resample_batch of this process read their weights (host-side bookkeeping):
 * the OR of PK2_RESAMPLE_PATH_LDS / _MEM over the jobs.  PK2_RESAMPLE_WEIGHTS=mem in the environment sends every job to
 * the memory path (measurements, tests). */
#define PK2_RESAMPLE_PATH_NONE 0
#define PK2_RESAMPLE_PATH_LDS 1
#define PK2_RESAMPLE_PATH_MEM 2
int pk2_resample_last_path(int32_t* path);

/* ------------------------------------------------------------------ *
 * Isotropic (diffuse) noise field for a microphone array (reference simulation/_iso_noise_simulator.py
 * `generate_isotropic_noise`, Habets & Gannot 2007).
 *   X[m][f] = (1 / sqrt(P)) sum_i g[f] Z_i[f] exp(-j tau[m][i] w_f),  w_f = 2 pi f / fft_size, fft_size = 2 (bins - 1),
 * then DC and Nyquist -> sqrt(fft_size) Re, the other bins * sqrt(fft_size / 2).  tau: device f64 (C, P) in samples;
 * g: device f64 (bins) or NULL (white); draws: device f32 (P, bins, 2) standard normals, or NULL: the counter-based
 * generator of pk2_iso_gauss(seed).  X: device f32 (C, bins, 2).  The sum over i runs in order in one thread:
 * bit-reproducible.
 * ------------------------------------------------------------------ */
int pk2_iso_spectra(const double* tau, const double* g, const float* draws, uint64_t seed, int32_t channels, int32_t points,
                    int32_t bins, float* X, void* stream);
/* out (P, bins, 2): the generator's draws, a pure function of (seed, i, f): splitmix64 finaliser of
 * seed * 0xD1342543DE82EF95 + i * bins + f, u1 / u2 = (k + 0.5) 2^-24 from bits 63..40 / 39..16, Box-Muller. */
int pk2_iso_gauss(uint64_t seed, int32_t points, int32_t bins, float* out, void* stream);

/* Inverse real FFT, numpy.fft.irfft normalisation: X (rows, n / 2 + 1) interleaved complex -> out (rows, n) real,
 * n = 2^5 .. 2^20.  The imaginary parts of DC and Nyquist are ignored.  out must not alias X. */
int pk2_irfft_pow2_f32(const float* X, int32_t rows, int32_t n, float* out, void* stream);

/* ------------------------------------------------------------------ *
 * Short-time Fourier transform, its inverse and ideal time-frequency masks (reference simulation/freq_analysis.py
 * `stft` / `istft` with center=False, simulation/mask.py `MaskEstimator`).  fft_size = 2^5 .. 2^12,
 * 1 <= frame_len <= fft_size, 1 <= frame_shift <= frame_len; window: device f32 (frame_len).  Spectra are FRAME-MAJOR:
 * (rows, N, F, 2) interleaved complex, F = fft_size / 2 + 1 (the reference's analyze returns (F, N)).
 * ------------------------------------------------------------------ */
/* N = ceil((n + frame_shift - frame_len) / frame_shift), the frames of _enframe(end='pad'); -1 when n < frame_len. */
int64_t pk2_stft_num_frames(int64_t n, int32_t frame_len, int32_t frame_shift);
/* rows: HOST array of R device pointers to signals of n samples each (n >= frame_len).  Frame = (x + dither) * window,
 * zero-extended to fft_size; the signal is zero-padded at its end to N whole frames.  dither: device f32 (R, n) that is
 * added, or NULL; with NULL and use_seed != 0 the generator of pk2_iso_gauss: the pair of (row r, sample pair p) is
 * draw r * ceil(n / 2) + p of `seed`, sample 2p takes its real and 2p + 1 its imaginary part, added as
 * x + fl(1e-5f * z) -- bit-equal to dither = 1e-5f * pk2_iso_gauss(seed, R, ceil(n / 2)).  out: (R, N, F, 2). */
int pk2_stft_f32(const float* const* rows, int32_t R, int64_t n, int32_t fft_size, int32_t frame_len, int32_t frame_shift,
                 const float* window, const float* dither, int32_t use_seed, uint64_t seed, float* out, void* stream);
/* X (R, N, F, 2) -> out (R, fft_size + frame_shift (N - 1)): per frame the inverse real transform, overlap-add (a gather
 * in frame order: bit-reproducible), divided by the summed analysis window (its frame_len taps) where that sum > 1e-10.
 * No synthesis window.  work: device f32 (R, N, fft_size). */
int pk2_istft_f32(const float* X, int32_t R, int32_t N, int32_t fft_size, int32_t frame_len, int32_t frame_shift,
                  const float* window, float* work, float* out, void* stream);
/* power[i] = |spec[i]|^2 over `count` complex values (the array pk2_mask_count_threshold reads). */
int pk2_mask_power(const float* spec, int64_t count, float* power, void* stream);
/* The cutoff of the 'count' clean mask for S arrays of m non-negative powers each (device f32 (S, m), m <= 2^27):
 * with the values sorted ascending and summed cumulatively in float64, v* = the last value whose inclusive sum is
 * < (1 - energy_threshold) * total, and the mask is power > v*.  out: device f32 (S, 3) = (v, strict, v*): keep
 * power > v when strict != 0, power >= v otherwise (v* is then v's predecessor).  No element satisfying the inequality
 * gives (min, 0, 0): everything is kept.  A radix descent over the bit pattern, no sort, independent of the order of
 * its atomics; nothing is read back.  work: device memory of pk2_mask_count_workspace_bytes(S) bytes. */
size_t pk2_mask_count_workspace_bytes(int32_t S);
int pk2_mask_count_threshold(const float* power, int32_t S, int64_t m, double energy_threshold, void* work, size_t work_bytes,
                             float* out, void* stream);
/* mask (S, N, F) of S clean spectra (S, N, F, 2) against one distorted spectrum (N, F, 2): with P_c = |C|^2,
 * soft == 0: P_c > snr_factor * max(|D - C|^2, FLT_EPSILON) (snr_factor = 10^(threshold_db / 10)); soft != 0:
 * min(1, P_c / |D|^2).  Times the clean-mask decision of thr (S, 3) = pk2_mask_count_threshold's output (NULL: all
 * ones) and of vad (N) > 0.5 per frame (NULL: all ones). */
int pk2_mask_ibm(const float* clean, const float* distorted, int32_t S, int32_t N, int32_t F, float snr_factor, int32_t soft,
                 const float* thr, const float* vad, float* mask, void* stream);

/* ------------------------------------------------------------------ *
 * Room impulse responses by the image method (reference simulation/_rirgen.py `xp_rirgen`, method 1), a batch of
 * items per call; the host checks the arguments and forms the descriptors (pykaldi2_amd/rirgen.py).  All arrays are
 * device memory.  Lengths are in samples (metres / (c / fs)).
 *   item_f64[i][PK2_RIR_F64]: room[3], beta[6], c0 = 0.5 / c * fs, gain threshold = (1 / c0) / 1e4, c / fs,
 *                             Habets high-pass b1, b2, a1, a2 (b0 = a0 = 1)
 *   item_i64[i][PK2_RIR_I64]: nsrc, nmic, nsamples, htw, high-pass (0 none, 1 FIR, 2 Habets IIR), first double of the
 *                             item's positions in `pos` (nsrc sources then nmic mics, xyz each), first float of the
 *                             item's rows in `out`, first row (index into `delay`), lattice half-widths ax, ay, az
 *                             (lattice points |x| <= ax ...; ax = min(int(nsamples / room[0]), int(nsamples / (2 room[0])) + 1)),
 *                             one spare
 *   wg[nwg][5]:               one workgroup each: item, row in the item (src * nmic + mic), part, number of parts (the
 *                             row's lattice points are split into that many equal ranges), first sample of the segment
 *                             (multiple of pk2_rirgen_segment_samples(); every (row, part, segment) once)
 *   row_item[nrows][2]:       item and row in the item of every row
 *   acc:                      workspace, int64[total] (zeroed here); out: f32[total], the rows (src, mic) of each item
 *                             back to back at its offset; delay: int32[nrows], argmax of each row (first maximum).
 * The result does not depend on the schedule: the taps are summed as 64-bit fixed point (bit-reproducible). */
#define PK2_RIR_F64 16
#define PK2_RIR_I64 12
int32_t pk2_rirgen_segment_samples(void);
int pk2_rirgen(const double* item_f64, const int64_t* item_i64, const double* pos, const int32_t* wg, int32_t nwg,
               const int32_t* row_item, int32_t nrows, int64_t total, void* acc, float* out, int32_t* delay,
               void* stream);

/* ------------------------------------------------------------------ *
 * 80-dim log-mel filterbank + CMN + frame subsampling.
 * Replaces DataGeneratorTrain._logfbank_extractor (reference
 * data/sr_dataset.py:279-296 over simulation/freq_analysis.py:113-150),
 * preprocess.cmn(axis=0) (reader/preprocess.py:34-41, called
 * data/sr_dataset.py:365-366) and the roll+unfold subsampling of
 * bin/train_chain.py:251-255.
 * ------------------------------------------------------------------ */
/* mel: host f32[80*257], the rows of data/mel80_window.txt (un-normalised);
 * the column normalisation of sr_dataset.py:283-286 is applied inside. */
typedef struct pk2_fbank pk2_fbank;
int pk2_fbank_create(const float* mel_80x257, pk2_fbank** out);
int pk2_fbank_destroy(pk2_fbank* fb);
/* wav: device f32, utterance n at wav[wav_off[n] .. wav_off[n+1]) (HOST int64
 * offsets).  feats: device f32 [sum_n frames[n]][80] packed in utterance order;
 * frames[n] = pk2_fbank_num_frames(samples).  feat_row_off: DEVICE int64
 * [num_utts+1] prefix sums of frames[] (row of each utterance's first frame).
 * If apply_cmn, the per-utterance mean over time is subtracted. */
int32_t pk2_fbank_num_frames(int64_t num_samples);
int pk2_fbank_compute(const pk2_fbank* fb, const float* wav, const int64_t* wav_off,
                      int32_t num_utts, float* feats, const int64_t* feat_row_off,
                      int32_t apply_cmn, void* stream);
/* Zero-pad to max_t, roll by `shift` (<=0, wraps like torch.roll) and keep
 * every `subsample`-th frame: x(n, j)[:] = feats_n[(j*subsample - shift) mod
 * max_t] (zero where that index >= frames[n]).  x is [num_utts][out_t][80], or
 * [out_t][num_utts][80] when time_major != 0 (the layout the LSTM kernels use). */
int pk2_pad_roll_subsample(const float* feats, const int64_t* feat_row_off, int32_t num_utts,
                           int32_t max_t, int32_t shift, int32_t subsample, float* x,
                           int32_t out_t, int32_t time_major, void* stream);

/* y = (x - mean) / std per feature dimension: GlobalMeanVarianceNormalization.apply_on_ndarray
 * (reference reader/preprocess.py:211-229, applied at data/sr_dataset.py:184-185).  x, y: device f32
 * [rows][dim]; mean, std: device f32 [dim]. */
int pk2_mvn_apply(const float* x, const float* mean, const float* stdv, int64_t rows, int32_t dim,
                  float* y, void* stream);

/* ------------------------------------------------------------------ *
 * SpecAugment (Park et al. 2019) on the packed feature rows of a ragged minibatch: time warp, then frequency and time
 * masks in output coordinates.  One launch on the caller's stream, no host synchronisation, no atomics.  No counterpart
 * in the reference; Kaldi's spec-augment-layer differs (which restates this contract).
 * in / out: device f32 [total_rows][80], the layout of pk2_fbank_compute; row_off: DEVICE int64 [n + 1] as there.
 * plan: DEVICE int32 [n][PK2_SPEC_PLAN_STRIDE]; the row of an utterance of T frames is
 *   c, d                                    the warp's centre and where it moves to (c == d: no warp)
 *   PK2_SPEC_MAX_FREQ_MASKS pairs (a, b)    half-open bin intervals, 0 <= a <= b <= 80
 *   PK2_SPEC_MAX_TIME_MASKS pairs (a, b)    half-open frame intervals, 0 <= a <= b <= T
 * unused intervals are (0, 0); intervals may overlap or be empty.
 * Warp (c != d; 1 <= c, d <= T - 2 keeps both denominators >= 1), output frame t, products in int64:
 *   t <= d: base = 0, num = t c, den = d;   else: base = c, num = (t - d)(T - 1 - c), den = T - 1 - d;
 *   i = base + num / den, r = num % den, a = in[i], b = in[min(i + 1, T - 1)];
 *   out[t] = a when r == 0, else fmaf((float)r / (float)den, b - a, a).
 * Frames 0 and T - 1 map to themselves; source indices are clamped into [0, T - 1], and a row whose den would not be
 * positive is copied, so no plan reads another utterance's rows.
 * Masks: out[t][f] = fill when t lies in any time interval or f in any frequency interval.
 * Elements that are neither masked nor interpolated are bit-exact copies (-0.0, denormals, NaN payloads included).
 * has_warp == 0: c and d are ignored; in == out is allowed, and then nothing is read and only masked elements are
 * written.  has_warp != 0 with in == out, or in and out overlapping without being equal: PK2_ERR_INVALID.  n < 1,
 * total_rows < n and null pointers: PK2_ERR_INVALID.
 * ------------------------------------------------------------------ */
#define PK2_SPEC_MAX_FREQ_MASKS 4
#define PK2_SPEC_MAX_TIME_MASKS 16
#define PK2_SPEC_PLAN_STRIDE (2 + 2 * PK2_SPEC_MAX_FREQ_MASKS + 2 * PK2_SPEC_MAX_TIME_MASKS)   /* int32 per utterance */
int pk2_spec_augment(const float* in, float* out, const int64_t* row_off /* device [n+1] */, int32_t n,
                     int64_t total_rows, const int32_t* plan /* device [n, STRIDE] */, int32_t has_warp,
                     float fill, void* stream);

/* ------------------------------------------------------------------ *
 * Mask-based MVDR beamforming of a ragged minibatch (csrc/beamform.hip; no counterpart in the reference).
 * B utterances with their own frame counts N_b and common C channels (1 .. PK2_BF_MAX_CHANNELS), F bins and K masks
 * (1 .. PK2_BF_MAX_MASKS).  Spectra are what pk2_stft_f32 writes for the C rows of one signal: (C, N_b, F, 2), channel- and
 * frame-major; masks are f32 (N_b, F).  `spec`, `masks`, `phi_s`, `phi_n`, `w` (of pk2_bf_apply) and `out` are HOST arrays
 * of device pointers, `frames` is a HOST array; more than PK2_BF_MAX_UTTS utterances take one launch per PK2_BF_MAX_UTTS.
 * No atomics, no host synchronisation: a result is bit-identical from run to run and independent of the other utterances
 * of its call.  Bad arguments (null pointers, B < 1, C, F, K or a frame count out of range, a workspace too small) return
 * PK2_ERR_INVALID before the device is touched.
 *
 * pk2_bf_cov: Phi_k[f] = sum_t m_k[t, f] y y^H / max(sum_t m_k[t, f], 1e-10), y = Y[:, t, f].  masks: B * K pointers,
 * utterance-major.  complement != 0 needs K == 1 and gives two matrices, for m and for 1 - m, from the same pass.
 * phi: device (B, K', F, C, C, 2), K' = complement ? 2 : K; exactly Hermitian (one triangle computed in float32 over
 * PK2_BF_FRAMES_PER_PART frames per workgroup, the parts added in order in float64, the other triangle mirrored; the
 * diagonal is real).
 *
 * pk2_bf_mvdr_weights (Souden): Phi_n' = Phi_n + (diag_load Re tr(Phi_n) / C + 1e-10) I, G = Phi_n'^-1 Phi_s (Cholesky, in
 * float64), w[f] = G[:, r] / tr G; w[f] = e_r where |tr G| <= 1e-20 or the bin's input is not finite (then nonfinite[b]
 * becomes 1, else 0).  phi_s, phi_n: B pointers to (F, C, C, 2) each.  ref = r in [0, C), or PK2_BF_REF_SNR:
 * r = argmax_c sum_f Re(w^(c)H Phi_s w^(c)) / sum_f Re(w^(c)H Phi_n' w^(c)), sums in bin order in float64, ties to the
 * lowest c, chosen on the device.  w: device (B, F, C, 2); ref_index, nonfinite: device int32 [B].
 *
 * pk2_bf_apply: out_b[t, f] = sum_c conj(w_b[f, c]) Y_b[c, t, f], c ascending in float32; out_b: (N_b, F, 2).
 *
 * work: device memory of pk2_bf_workspace_bytes(frames, B, C, F, K, complement) bytes, enough for pk2_bf_cov and
 * pk2_bf_mvdr_weights of that minibatch (frames == NULL: for pk2_bf_mvdr_weights alone; K and complement are then
 * ignored); 0 for arguments the entries would refuse.
 * ------------------------------------------------------------------ */
#define PK2_BF_MAX_CHANNELS 8
#define PK2_BF_MAX_MASKS 4
#define PK2_BF_MAX_UTTS 32
#define PK2_BF_FRAMES_PER_PART 32
#define PK2_BF_REF_SNR (-1)
size_t pk2_bf_workspace_bytes(const int32_t* frames, int32_t B, int32_t C, int32_t F, int32_t K, int32_t complement);
int pk2_bf_cov(const float* const* spec, const float* const* masks, const int32_t* frames, int32_t B, int32_t C, int32_t F,
               int32_t K, int32_t complement, void* work, size_t work_bytes, float* phi, void* stream);
int pk2_bf_mvdr_weights(const float* const* phi_s, const float* const* phi_n, int32_t B, int32_t C, int32_t F, int32_t ref,
                        double diag_load, void* work, size_t work_bytes, float* w, int32_t* ref_index, int32_t* nonfinite,
                        void* stream);
int pk2_bf_apply(const float* const* spec, const float* const* w, const int32_t* frames, int32_t B, int32_t C, int32_t F,
                 float* const* out, void* stream);

/* ------------------------------------------------------------------ *
 * WPE dereverberation of a ragged minibatch (csrc/wpe.hip; no counterpart in the reference): weighted
 * prediction error, multi-channel linear prediction per frequency bin.  B utterances with their own frame counts N_b and
 * common C channels (1 .. PK2_WPE_MAX_CHANNELS), F bins, K = taps and a prediction delay (1 .. PK2_WPE_MAX_DELAY);
 * D = C K <= PK2_WPE_MAX_ORDER.  Spectra are (C, N_b, F, 2) as for the beamformer.  The stacked past of frame t is
 * y~(t)[k C + c] = Y[c, t - delay - k, f], zero before the first frame.  `spec`, `weight`, `power`, `out` and `power_out`
 * are HOST arrays of device pointers, `frames` is a HOST array; more than PK2_WPE_MAX_UTTS utterances take one launch per
 * PK2_WPE_MAX_UTTS.  No atomics, no host synchronisation: a result is bit-identical from run to run and independent of
 * the other utterances of its call.  Bad arguments return PK2_ERR_INVALID before the device is touched.
 *
 * pk2_wpe_power: power_b[t, f] = max((sum_c |Y[c, t, f]|^2) / C, 1e-10), the sum a float32 fmaf chain over c (re, then im).
 *
 * pk2_wpe_corr: R[f] = sum_t y~ y~^H / weight[t, f] (D x D), P[f] = sum_t y~ Y(t)^H / weight[t, f] (D x C).  The rows are
 * multiplied by the float32 reciprocal of the weight.  Frames are split into parts of PK2_WPE_FRAMES_PER_PART; a part is a
 * float32 chain in frame order on the f32 MFMA, the parts are added in part order in float64 and rounded once.  R is
 * exactly Hermitian with a real diagonal.  R: device (B, F, D, D, 2); P: device (B, F, D, C, 2).
 *
 * pk2_wpe_solve: R' = R + (diag_load Re tr R / D + 1e-10) I, G = R'^-1 P by Cholesky in float64, rounded once.  A bin whose
 * R or P is not finite, or whose factorisation or solution is not (R' not positive definite), gets G = 0 and sets
 * nonfinite[b] = 1 (else 0).  G: device (B, F, D, C, 2); nonfinite: device int32 [B].
 *
 * pk2_wpe_filter: out_b[c, t, f] = Y[c, t, f] - sum_d conj(G[f, d, c]) y~(t)[d], float32 fmaf chains in ascending d.
 * A bin whose G is all zero is copied, so it passes through bit for bit even where its past holds a NaN.
 * power_out (NULL, or B pointers to (N_b, F)): pk2_wpe_power of `out`, from the same pass.  out must not alias spec.
 *
 * pk2_wpe: X^0 = Y; iteration i = 1 .. iters: weight = power of X^(i-1), corr, solve, X^i = filter of Y.  out_b = X^iters;
 * nonfinite[b] = 1 when a bin of any iteration was not finite.  Nothing is read back.
 *
 * work: device memory of pk2_wpe_workspace_bytes(frames, B, C, F, taps, delay) bytes, enough for every entry on that
 * minibatch; 0 for arguments the entries would refuse.
 * ------------------------------------------------------------------ */
#define PK2_WPE_MAX_CHANNELS 8
#define PK2_WPE_MAX_ORDER 80
#define PK2_WPE_MAX_DELAY 8
#define PK2_WPE_MAX_ITERS 8
#define PK2_WPE_MAX_UTTS 32
#define PK2_WPE_FRAMES_PER_PART 1024
size_t pk2_wpe_workspace_bytes(const int32_t* frames, int32_t B, int32_t C, int32_t F, int32_t taps, int32_t delay);
int pk2_wpe_power(const float* const* spec, const int32_t* frames, int32_t B, int32_t C, int32_t F, float* const* power,
                  void* stream);
int pk2_wpe_corr(const float* const* spec, const float* const* weight, const int32_t* frames, int32_t B, int32_t C, int32_t F,
                 int32_t taps, int32_t delay, void* work, size_t work_bytes, float* R, float* P, void* stream);
int pk2_wpe_solve(const float* R, const float* P, int32_t B, int32_t C, int32_t F, int32_t taps, double diag_load, void* work,
                  size_t work_bytes, float* G, int32_t* nonfinite, void* stream);
int pk2_wpe_filter(const float* const* spec, const float* G, const int32_t* frames, int32_t B, int32_t C, int32_t F,
                   int32_t taps, int32_t delay, float* const* out, float* const* power_out, void* stream);
int pk2_wpe(const float* const* spec, const int32_t* frames, int32_t B, int32_t C, int32_t F, int32_t taps, int32_t delay,
            int32_t iters, double diag_load, void* work, size_t work_bytes, float* const* out, int32_t* nonfinite,
            void* stream);

/* ------------------------------------------------------------------ *
 * cGMM mask estimation of a ragged minibatch (csrc/cgmm.hip; no counterpart in the reference): per bin an
 * EM over the frames of a mixture of K complex Gaussians y ~ N(0, phi_k[t] R_k) with weights alpha_k (Higuchi et al. 2016),
 * optionally guided by a per-class frame activity.  B utterances with their own frame counts N_b and common C channels
 * (1 .. PK2_BF_MAX_CHANNELS), F bins and K classes (2 .. PK2_BF_MAX_MASKS).  Spectra are (C, N_b, F, 2) as for the
 * beamformer; masks, `init`, `lam` and `phi` planes are f32 (K, N_b, F); `activity` is f32 (K, N_b), >= 0, or NULL (all
 * ones).  `spec`, `init`, `activity`, `masks`, `lam` and `phi` are HOST arrays of B device pointers, `frames` is a HOST
 * array; more than PK2_BF_MAX_UTTS utterances take one launch per stage per PK2_BF_MAX_UTTS.  R: device (B, K, F, C, C, 2),
 * exactly Hermitian with a real diagonal; log_alpha: device (B, K, F).  No atomics, no host synchronisation: a result is
 * bit-identical from run to run and independent of the other utterances of its call.  Bad arguments return
 * PK2_ERR_INVALID before the device is touched.
 *
 * M-step (pk2_cgmm_update): R_k[f] = sum_t (lam_k / phi_k) y y^H / max(sum_t lam_k, 1e-10), summed as pk2_bf_cov sums;
 * alpha_k[f] = max(sum_t lam_k / max(N_act, 1), 1e-10), N_act the number of frames with an active class.
 *
 * pk2_cgmm_init: init == NULL (K = 2): R_0 = sum_t y y^H / N, R_1 = (Re tr R_0 / C) I, alpha = 1 / 2; else the M-step
 * with lam = init and phi = 1.
 *
 * pk2_cgmm_factor: R' = R + (diag_load Re tr R / C + 1e-10) I = L L^H in float64; linv (B, K, C (C + 1), F): the lower
 * triangle of L^-1 row by row as (re, im) planes over the bins, rounded once; bias (B, K, F) = log alpha - 2 sum log L_jj.
 * bad (B, K, F) int32: 1 where R is not finite or R' not positive definite (then L^-1 = I, bias = 0); nonfinite[b]: any.
 *
 * pk2_cgmm_posteriors: z = L^-1 y (fmaf chains, ascending column), q = sum |z_j|^2, phi_k = max(q / C, 1e-10),
 * l_k = bias_k + log a_k[t] - C log phi_k, lam = softmax_k l_k.  A class with a_k[t] = 0 gets lam = 0, a frame without an
 * active class lam = 0 for every class; a bin with a bad class lam = 1 / K on every frame.  ll[b] = the float64 sum over
 * t and f of max_k l_k + log sum_k exp(l_k - max) (frames without an active class and bad bins add nothing).
 *
 * pk2_cgmm: init, then iters (1 .. PK2_CGMM_MAX_ITERS) times factor, posteriors, M-step.  masks_b (K, N_b, F): the lam of
 * the last posteriors; R and log_alpha: the M-step of those; ll: device f64 (B, iters); nonfinite[b] = 1 when a bin of any
 * iteration was bad.  purity != 0 (K = 2): per bin, class 0 becomes the class with the larger ||R_k||_F^2 / (Re tr R_k)^2
 * (a tie keeps the order; a swap exchanges masks, R and log_alpha of that bin).
 *
 * work: device memory of pk2_cgmm_workspace_bytes(frames, B, C, F, K) bytes, enough for every entry on that minibatch; 0
 * for arguments the entries would refuse.
 * ------------------------------------------------------------------ */
#define PK2_CGMM_MAX_ITERS 32
size_t pk2_cgmm_workspace_bytes(const int32_t* frames, int32_t B, int32_t C, int32_t F, int32_t K);
int pk2_cgmm_init(const float* const* spec, const float* const* init, const float* const* activity, const int32_t* frames,
                  int32_t B, int32_t C, int32_t F, int32_t K, void* work, size_t work_bytes, float* R, float* log_alpha,
                  void* stream);
int pk2_cgmm_factor(const float* R, const float* log_alpha, int32_t B, int32_t C, int32_t F, int32_t K, double diag_load,
                    float* linv, float* bias, int32_t* bad, int32_t* nonfinite, void* stream);
int pk2_cgmm_posteriors(const float* const* spec, const float* const* activity, const int32_t* frames, int32_t B, int32_t C,
                        int32_t F, int32_t K, const float* linv, const float* bias, const int32_t* bad, void* work,
                        size_t work_bytes, float* const* lam, float* const* phi, double* ll, void* stream);
int pk2_cgmm_update(const float* const* spec, const float* const* lam, const float* const* phi, const float* const* activity,
                    const int32_t* frames, int32_t B, int32_t C, int32_t F, int32_t K, void* work, size_t work_bytes, float* R,
                    float* log_alpha, void* stream);
int pk2_cgmm(const float* const* spec, const float* const* init, const float* const* activity, const int32_t* frames, int32_t B,
             int32_t C, int32_t F, int32_t K, int32_t iters, double diag_load, int32_t purity, void* work, size_t work_bytes,
             float* const* masks, float* R, float* log_alpha, double* ll, int32_t* nonfinite, void* stream);

/* ------------------------------------------------------------------ *
 * Frequency permutation alignment of cGMM masks of a ragged minibatch (csrc/perm_align.hip; no counterpart
 * in the reference): a blind EM runs per bin, so its classes are unrelated from bin to bin; this finds one permutation
 * pi_f of the K classes (2 .. PK2_BF_MAX_MASKS) per bin from how the posteriors move over time (Sawada et al. 2011) and
 * writes out_masks_b[a, t, f] = masks_b[pi_f[a], t, f], out of place.  masks, out_masks: HOST arrays of B device pointers
 * to f32 (K, N_b, F); frames: HOST array.  cov (B, K, F, C, C, 2) and log_alpha (B, K, F), device, are optional (both or
 * neither, with out_cov and out_log_alpha) and are gathered the same way.  perm: device int32 (B, F, K) = pi_f[a];
 * margin: device f32 (B, F).
 *
 * u[f][k] = pearson(masks[k, :, f]), pearson(v) = (v - mean v) / max(||v - mean v||_2, 1e-10), float64 sums, stored as
 * f32 (F, K, N_b).  best(S) of a K x K score matrix: the permutation p maximising sum_a S[a][p[a]], the K! candidates in
 * lexicographic order, the first maximum wins.  Tree: level 0 has one group per bin (centroid u[f], weight 1); a level
 * merges the neighbours (2j, 2j + 1): S[a][b] = <cL[a], cR[b]>, p = best(S), every bin of the right group gets
 * pi_f <- pi_f o p (new pi_f[a] = old pi_f[p[a]]), the merged centroid is pearson(wL cL[a] + wR cR[p[a]]) with weight
 * wL + wR; a last odd group passes up.  Then `refine` (1 .. PK2_PERM_ALIGN_MAX_REFINE) rounds:
 * c[a] = pearson(sum_f u[f][pi_f[a]]); per bin S[a][b] = <c[a], u[f][pi_f[b]]>, p = best(S), pi_f <- pi_f o p.
 * margin[f]: the best score minus the second best of the last round.  noise_last != 0 with cov: the stream with the
 * smallest sum over the bins of ||R||_F^2 / (Re tr R)^2 (where finite) moves to position K - 1 (a tie keeps the first),
 * the others keep their order.  No atomics, no host synchronisation: bit-identical from run to run and independent of the
 * other utterances of the call; more than PK2_BF_MAX_UTTS utterances take one launch per stage per PK2_BF_MAX_UTTS.
 * work: device memory of pk2_perm_align_workspace_bytes(frames, B, F, K) bytes; 0 for arguments the entry would refuse.
 * ------------------------------------------------------------------ */
#define PK2_PERM_ALIGN_MAX_REFINE 8
size_t pk2_perm_align_workspace_bytes(const int32_t* frames, int32_t B, int32_t F, int32_t K);
int pk2_perm_align(const float* const* masks, const float* cov, const float* log_alpha, const int32_t* frames, int32_t B,
                   int32_t C, int32_t F, int32_t K, int32_t refine, int32_t noise_last, void* work, size_t work_bytes,
                   float* const* out_masks, float* out_cov, float* out_log_alpha, int32_t* perm, float* margin, void* stream);

/* ------------------------------------------------------------------ *
 * Lattice scoring (csrc/lattice_score.hip): what the reference's example/.../local/score.sh hand to Kaldi
 * (lattice-scale | lattice-add-penalty | lattice-best-path, lattice-mbr-decode, utt_wer.py), for a grid of
 * (lattice, setting) pairs per call.  A setting is three doubles (lm, am, wip): cost_a = lm graph_a + am acoustic_a +
 * wip [word_a != 0] in float64; `settings` is a HOST array of G x 3, G in 1 .. PK2_WORDLAT_MAX_SETTINGS.
 *
 * pk2_wordlat_create uploads N packed word lattices (all arguments HOST arrays; pykaldi2_amd/score.py: pack_lattice).
 * Per lattice: states 0..S-1 ordered by (level, id), level = longest arc count from the start, 0 = start, S-1 = the only
 * end; arcs sorted by (destination, original index).  state_off, arc_off (N + 1): offsets into the concatenated arrays;
 * level_off_off: offsets of the per-lattice level_off (depth + 2 entries: the state range of every level);
 * word_off_off: offsets of word_off (W + 1 entries; word_ids holds W entries per lattice, at word_off_off[n] - n).
 * src, dst, word (LOCAL id 0..W-1, 0 = epsilon, ascending with the word id), graph, acoustic: per arc; in_off, out_off
 * (S + 1 per lattice, at state_off[n] + n): CSR by destination (arcs are contiguous) and by source over out_idx (arc
 * indices, ascending); word_arcs: the arcs of every local word, ascending.  Every index is validated on the host; a
 * malformed lattice is PK2_ERR_INVALID.  The row capacity of a lattice is min(PK2_WORDLAT_MAX_POSITIONS, 2 depth + 1).
 *
 * Results are indexed by pair = (n - first) * G + g.  Failures of a pair are reported in status[pair] (0 ok, 1 not
 * converged, 2 capacity, 3 empty or failed), never through the return code.  Null pointers, G outside
 * 1 .. PK2_WORDLAT_MAX_SETTINGS, bins outside 0 .. PK2_WORDLAT_MAX_BINS, max_iter < 1, a non-finite scale, a range outside the
 * batch, strides below what the range needs and a short workspace return PK2_ERR_INVALID before the device is touched.
 * work: device memory of pk2_wordlat_workspace_bytes(h, first, count, G, bins) bytes (bins = -1: best path only; 0 for
 * arguments the entries would refuse).  No floating-point atomics, fixed summation orders: the same bits from run to
 * run and in a batch as in a single call.
 *
 * pk2_wordlat_best_path: alpha (log-add in incoming-arc order), arc posteriors, the tropical best path (a later arc
 * replaces an earlier one only on <).  words (pairs x word_stride, word_stride >= depth of every lattice of the range),
 * nwords, cost, alpha_end, status: device, per pair.  post (optional): p_a at G * (arc_off[n] - arc_off[first]) + g * A_n;
 * backpointer (optional): the best incoming arc of every state, at G * (state_off[n] - state_off[first]) + g * S_n.
 *
 * pk2_wordlat_mbr: minimum Bayes risk decoding (Xu, Povey, Mangu, Zhu 2011; DESIGN.md 7.13 fixes the arithmetic), started
 * from the best path, at most max_iter E-steps; decode_mbr = 0: one E-step on the best path and no update.  words, conf
 * (pairs x word_stride, word_stride >= (capacity - 1) / 2), nwords, risk, iterations, status per pair.  bins > 0: bin_n
 * per pair and bin_word / bin_post (pairs x bin_stride x bins, bin_stride >= capacity): for every position whose top
 * entry is not epsilon the `bins` highest (word, posterior) pairs, word -1 where the lattice has fewer words.
 *
 * Word times.  pk2_wordlat_set_times takes the frame at which every packed state is reached (HOST int32,
 * laid out like state_off: state_off[N] entries), checks on the host that every lattice starts at frame 0 and that no
 * arc has a negative length (PK2_ERR_INVALID otherwise) and uploads it once for the batch.  pk2_wordlat_mbr_times is
 * pk2_wordlat_mbr -- the same words, confidences, risk, iterations, status and bins, bit for bit -- followed by the time
 * statistics of the last E-step: times (pairs x word_stride x 2): (begin, end) of every hypothesis word in frames,
 * TB / gamma and TE / gamma with TB(q)[w] = sum over the arcs of w of [dec_a(q) = 1] t(s_a) b_a(q) and TE with t(n_a),
 * (-1, -1) where gamma <= 0; bin_times (pairs x bin_stride x bins x 2, with bins > 0): the same for every bin entry,
 * (-1, -1) for epsilon and for absent entries; path_times (pairs x path_stride x 2, path_stride >= depth of every
 * lattice of the range): (t(s_a), t(n_a)) of the word arcs of the best path, the rows behind them (-1, -1).  work:
 * pk2_wordlat_times_workspace_bytes(h, first, count, G, bins) bytes.  A batch without uploaded times, null outputs and a
 * short path_stride or workspace are refused before the device is touched.
 *
 * pk2_edit_distance_batch: Levenshtein distance with unit costs of n pairs, one wavefront each; hyp / ref: device int32
 * labels, hyp_off / ref_off: device int64 (n + 1); out[i] = -1 for a reference beyond PK2_WORDLAT_MAX_POSITIONS labels.
 * ------------------------------------------------------------------ */
#define PK2_WORDLAT_MAX_SETTINGS 64
#define PK2_WORDLAT_MAX_POSITIONS 1023
#define PK2_WORDLAT_MAX_BINS 8
int pk2_wordlat_create(int32_t N, const int64_t* state_off, const int64_t* arc_off, const int64_t* level_off_off,
                       const int64_t* word_off_off, const int32_t* src, const int32_t* dst, const int32_t* word,
                       const float* graph, const float* acoustic, const int32_t* in_off, const int32_t* out_off,
                       const int32_t* out_idx, const int32_t* level_off, const int32_t* word_ids, const int32_t* word_off,
                       const int32_t* word_arcs, void* stream, void** out);
int pk2_wordlat_destroy(void* h);
size_t pk2_wordlat_workspace_bytes(const void* h, int32_t first, int32_t count, int32_t G, int32_t bins);
int pk2_wordlat_best_path(const void* h, int32_t first, int32_t count, const double* settings, int32_t G, void* work,
                          size_t work_bytes, int32_t* words, int32_t word_stride, int32_t* nwords, double* cost, double* alpha_end,
                          double* post, int32_t* backpointer, int32_t* status, void* stream);
int pk2_wordlat_mbr(const void* h, int32_t first, int32_t count, const double* settings, int32_t G, int32_t decode_mbr,
                    int32_t max_iter, int32_t bins, void* work, size_t work_bytes, int32_t* words, double* conf,
                    int32_t word_stride, int32_t* nwords, double* risk, int32_t* iterations, int32_t* status, int32_t* bin_n,
                    int32_t* bin_word, double* bin_post, int32_t bin_stride, void* stream);
int pk2_wordlat_set_times(void* h, const int32_t* state_time);
size_t pk2_wordlat_times_workspace_bytes(const void* h, int32_t first, int32_t count, int32_t G, int32_t bins);
int pk2_wordlat_mbr_times(const void* h, int32_t first, int32_t count, const double* settings, int32_t G, int32_t decode_mbr,
                          int32_t max_iter, int32_t bins, void* work, size_t work_bytes, int32_t* words, double* conf,
                          int32_t word_stride, int32_t* nwords, double* risk, int32_t* iterations, int32_t* status,
                          int32_t* bin_n, int32_t* bin_word, double* bin_post, int32_t bin_stride, double* times,
                          double* bin_times, int32_t* path_times, int32_t path_stride, void* stream);
int pk2_edit_distance_batch(const int32_t* hyp, const int64_t* hyp_off, const int32_t* ref, const int64_t* ref_off, int32_t n,
                            int32_t* out, void* stream);

/* ------------------------------------------------------------------ *
 * MBR system combination (csrc/lattice_combine.hip): the reference's score_combine.sh (lattice-combine |
 * lattice-mbr-decode) on a pk2_wordlat_create batch whose lattices are stored group by group, a group = the lattices that
 * K systems (1 .. PK2_WORDLAT_MAX_SYSTEMS) made of one utterance.  The union's path distribution is sum_k wn_k P_k with
 * P_k the path posterior of system k under the setting; no union lattice is built: every system runs the E-step of
 * pk2_wordlat_mbr on its own lattice and the statistics are added with the weights, in ascending k.
 *
 * pk2_wordlat_set_groups (all arguments HOST arrays, uploaded once): group_off (NG + 1) the lattice range of every group;
 * wn, log_wn (N): the normalised weight of every lattice within its group (positive, adding up to 1 per group) and its
 * logarithm -- both are passed so that the device and a restatement use the same numbers; uvoc_off (NG + 1), uvoc: the
 * ascending union of the group's word ids, 0 first; map: for every lattice, in batch order, one entry per word of its
 * group's vocabulary: the lattice's LOCAL id of that word, or W (its number of local words) for a word it does not have.
 * Everything is validated on the host (PK2_ERR_INVALID).  The row capacity of a group is
 * min(PK2_WORDLAT_MAX_POSITIONS, 2 max depth + 1); every system's rows have that size.
 *
 * pk2_wordlat_combine decodes the groups first_group .. first_group + group_count - 1 under G settings; results are indexed
 * by pair = (group - first_group) * G + g and are those of pk2_wordlat_mbr (words, conf: pairs x word_stride, word_stride >=
 * (capacity - 1) / 2 of every group; bins: bin_stride >= capacity) plus system[pair]: the system (index within the group)
 * whose best path was the first hypothesis -- the one minimising v_k(end) + alpha_k(end) - log wn_k, a later system on <
 * only; -1 with status 3.  status: 0 ok, 1 not converged within max_iter E-steps, 2 capacity, 3 a system of the group has no
 * finite alpha(end).  max_iter in 1 .. PK2_WORDLAT_COMBINE_MAX_ITER: 2 max_iter + 2 launches are enqueued, nothing is read
 * back.  work: device memory of pk2_wordlat_combine_workspace_bytes(h, first_group, group_count, G, bins) bytes (0 for
 * arguments the entry would refuse).  The same bits from run to run, for a group in a batch as alone, and for a group of
 * one system as pk2_wordlat_mbr of that lattice.
 * ------------------------------------------------------------------ */
#define PK2_WORDLAT_MAX_SYSTEMS 8
#define PK2_WORDLAT_COMBINE_MAX_ITER 100
int pk2_wordlat_set_groups(void* h, int32_t NG, const int32_t* group_off, const double* wn, const double* log_wn,
                           const int64_t* uvoc_off, const int32_t* uvoc, const int32_t* map);
size_t pk2_wordlat_combine_workspace_bytes(const void* h, int32_t first_group, int32_t group_count, int32_t G, int32_t bins);
int pk2_wordlat_combine(const void* h, int32_t first_group, int32_t group_count, const double* settings, int32_t G,
                        int32_t decode_mbr, int32_t max_iter, int32_t bins, void* work, size_t work_bytes, int32_t* words,
                        double* conf, int32_t word_stride, int32_t* nwords, double* risk, int32_t* iterations, int32_t* status,
                        int32_t* system, int32_t* bin_n, int32_t* bin_word, double* bin_post, int32_t bin_stride, void* stream);

/* ------------------------------------------------------------------ *
 * Lattice oracle (csrc/lattice_oracle.hip): Kaldi's lattice-oracle on a pk2_wordlat_create batch -- the
 * smallest edit distance (unit costs) between a reference and any path of the lattice, the path that reaches it and its
 * insertions, deletions and substitutions; one workgroup per lattice, integers only, no settings.
 *
 * arc_label: DEVICE int32 laid out like arc_off of the whole batch: 0 for an arc that costs nothing (epsilon, or a word
 * the caller wants skipped), otherwise the arc's local word id.  ref: DEVICE int32, the references of the range in the
 * lattices' LOCAL word ids, -1 for a word a lattice does not contain (it never matches); ref_off (DEVICE) and ref_off_host
 * (HOST), count + 1 entries each and equal: the reference of lattice first + i is ref[ref_off[i] .. ref_off[i + 1]).
 *   D[0][j] = j;  C[n][j] = min over the incoming arcs a = (s -> n) of  label_a == 0: D[s][j];  otherwise
 *   min(D[s][j] + 1, D[s][j-1] + (label_a != ref[j-1]));  D[n][j] = min over k <= j of C[n][k] + (j - k);
 *   errors = D[S-1][R].
 * The path is walked back from (S-1, R): at (n, j) the incoming arcs of n in ascending index, for each first the diagonal
 * step, then the free step, then the insertion; the first arc that fits is taken, and if none fits the step is a deletion
 * to (n, j-1).  Outputs per lattice of the range (device): errors; counts (3: insertions, deletions, substitutions, their
 * sum = errors); words (word_stride per lattice: the GLOBAL ids of the path's labels != 0, the rest -1) and nwords; path
 * (path_stride per lattice: the packed arc indices of the path, the rest -1) and npath; status: 0 ok, 2 a reference of
 * more than PK2_WORDLAT_MAX_POSITIONS words (errors -1, words and path all -1, nothing else written), 3 failed (the same;
 * device offsets that disagree with ref_off_host end here and write nothing to the workspace).
 * work: device memory of pk2_wordlat_oracle_workspace_bytes(h, first, count, ref_off_host) bytes (0 for arguments the
 * entry would refuse): per lattice (S + 64) x (R + 1) + 2 depth int32.  Null pointers, a range outside the batch, a
 * negative or decreasing ref_off_host, word_stride or path_stride below the depth of a lattice of the range and a short
 * or misaligned workspace return PK2_ERR_INVALID before the device is touched.  The same bytes for a lattice alone, in a
 * batch and in any split of the batch into calls.
 * ------------------------------------------------------------------ */
size_t pk2_wordlat_oracle_workspace_bytes(const void* h, int32_t first, int32_t count, const int64_t* ref_off);
int pk2_wordlat_oracle(const void* h, int32_t first, int32_t count, const int32_t* arc_label, const int32_t* ref,
                       const int64_t* ref_off, const int64_t* ref_off_host, void* work, size_t work_bytes, int32_t* errors,
                       int32_t* counts, int32_t* words, int32_t word_stride, int32_t* nwords, int32_t* path,
                       int32_t path_stride, int32_t* npath, int32_t* status, void* stream);

/* ------------------------------------------------------------------ *
 * Word-boundary alignment of best-path word times (csrc/lattice_align_words.hip): what the recipes'
 * `lattice-1best | lattice-align-words word_boundary.int final.mdl | nbest-to-ctm` (and lattice-align-phones) print, for
 * every (lattice, setting) pair of a pk2_wordlat_best_path call; one workgroup per pair, integers only.
 *
 * pk2_wordlat_set_strings gives a pk2_wordlat_create batch the transition-id string of every packed arc: tid_off (HOST
 * int64, arc_off[N] + 1 entries, laid out like arc_off: the string of arc a of lattice n is tids[tid_off[arc_off[n] + a] ..
 * tid_off[arc_off[n] + a + 1])) and tids (HOST int32).  Offsets that do not start at 0 or decrease and a transition-id
 * below 1 are PK2_ERR_INVALID.  It records the largest transition-id and per lattice its frame capacity -- the longest
 * start -> end path in frames (below 2^30), pk2_wordlat_frame_capacity copies them to a HOST int32[N] -- and uploads once;
 * a second call is refused.
 *
 * pk2_wordalign_model_create holds the tables on the device: tid_tstate, tid_phone, tid_flags as pk2_split_to_phones takes
 * them (num_tids + 1 entries, entry 0 unused; bit 0 self-loop, bit 1 transition to the final HMM state) and phone_cat
 * (uint8, num_phones entries indexed by phone: 0 nonword, 1 begin, 2 end, 3 internal, 4 singleton, 255 no entry; a phone
 * >= num_phones has no entry).
 *
 * pk2_wordlat_align_words: backpointer and bp_status are the DEVICE outputs `backpointer` and `status` of a
 * pk2_wordlat_best_path call on the same range with the same G, in the same stream.  Per pair = (n - first) * G + g:
 *   the path's arcs follow the back-pointers from the end state; its string is the concatenation of their strings, an
 *   arc begins at the sum of the lengths before it.  path_times (pairs x word_stride x 2): (begin, begin + length) of the
 *   j-th arc with a word label, the rows behind them (-1, -1).
 *   phones (optional; pairs x phone_stride x 3: phone, begin, duration) and nphones: exactly pk2_split_to_phones on the
 *   path's string; its *ok = 0 sets bit 1 of reason.
 *   tokens (pairs x token_stride x 4: label, begin, duration, kind) and ntokens: with c_k the category of phone k, phone k
 *   starts a token when k = 0, c_k is nonword, singleton or begin, or c_{k-1} is nonword, singleton or end.  kind 0: a
 *   silence (one nonword phone); 1: a word (one singleton phone, or begin internal* end); 2: partial (anything else; bit 2
 *   of reason).  label: the path's j-th word label on the j-th token of kind 1 or 2, otherwise 0.
 *   word_times (pairs x word_stride x 2): (begin, end) of the j-th token of kind 1 or 2; rows behind the words (-1, -1).
 *   status 0 when reason = 0; reason bit 4: the number of such tokens differs from the number of word labels; bit 8: a
 *   phone without a category.  status 1 otherwise: word_times is then a copy of path_times.  status 3: bp_status != 0 or a
 *   back-pointer that is not an arc into its state; nothing but (-1, -1) rows and zero counts is written.
 * word_stride >= the depth of every lattice of the range; token_stride, phone_stride >= its frame capacity.  work: device
 * memory of pk2_wordlat_align_workspace_bytes(h, first, count, G) bytes (0 for arguments the entry would refuse), per pair
 * 3 depth + 4 capacity int32.  Null pointers (phones may be null), a batch without strings, a largest transition-id above
 * the model's num_tids, G outside 1 .. PK2_WORDLAT_MAX_SETTINGS, a range outside the batch, short strides and a short or
 * misaligned workspace return PK2_ERR_INVALID before the device is touched; failures of a pair go to status.  The same
 * bits for a lattice alone, in a batch and in any split of the batch into calls.
 * ------------------------------------------------------------------ */
int pk2_wordlat_set_strings(void* h, const int64_t* tid_off, const int32_t* tids);
int pk2_wordlat_frame_capacity(const void* h, int32_t* out);
int pk2_wordalign_model_create(int32_t num_tids, const int32_t* tid_tstate, const int32_t* tid_phone, const uint8_t* tid_flags,
                               int32_t num_phones, const uint8_t* phone_cat, void* stream, void** out);
int pk2_wordalign_model_destroy(void* model);
size_t pk2_wordlat_align_workspace_bytes(const void* h, int32_t first, int32_t count, int32_t G);
int pk2_wordlat_align_words(const void* h, const void* model, int32_t first, int32_t count, int32_t G,
                            const int32_t* backpointer, const int32_t* bp_status, void* work, size_t work_bytes,
                            int32_t* path_times, int32_t* word_times, int32_t word_stride, int32_t* tokens, int32_t* ntokens,
                            int32_t token_stride, int32_t* phones, int32_t* nphones, int32_t phone_stride, int32_t* status,
                            int32_t* reason, void* stream);

/* ------------------------------------------------------------------ *
 * N-gram LM rescoring of word lattices (csrc/lattice_lmrescore.hip): what the reference's
 * local/lmrescore_const_arpa.sh hands to Kaldi (lattice-lmrescore | lattice-lmrescore-const-arpa) -- the composition of a
 * packed word lattice with a deterministic backoff LM, one workgroup per lattice.
 *
 * pk2_ngram_create uploads the trie of pykaldi2_amd/ngram.py (all arguments HOST arrays).  N nodes: node 0 = the empty
 * history, then the unigrams in ascending word id, then the order-k n-grams sorted by (parent node, word); order_off
 * (order + 2): the node range of every order (order_off[0] = 0, order_off[1] = 1).  Per node: word, cost = -ln p, backoff =
 * -ln bo (0 where absent), child_begin (N + 1: the children of node i are child_begin[i] .. child_begin[i + 1]),
 * bo_link (the longest proper suffix that is a node), next_state (the longest suffix of at most order - 1 words with
 * children, or 0).  start: the LM state after <s>; eos: the word id of </s>.  Validated on the host before the upload:
 * child ranges monotone and inside the next order, words ascending inside a child range, bo_link to a strictly lower
 * order, next_state and start a node with children or 0, finite weights, a unigram for eos; otherwise PK2_ERR_INVALID.
 *
 * pk2_wordlat_lmrescore composes the lattices first .. first + count - 1 of a pk2_wordlat_create batch with the LM:
 * states = the reachable pairs (packed state s, LM node h) numbered in ascending (s, h), arcs in ascending (destination
 * pair, input arc, source pair); an arc along input arc a from (s, h): into the end state cost = final(h), target
 * (S - 1, 0); another epsilon cost 0, target (n_a, h); a word arc (cost, h') = arc(h, lm_word[word_a]), target
 * (n_a, h'); new graph cost = float32(float64(graph_a) + scale * cost) with separate roundings.  lm_word: DEVICE array laid
 * out like word_ids of the whole batch: the LM's word id of every local word (a word without a unigram: status 3).
 * Lattice i of the range has room for (int64)(expand * S_i) states and (int64)(expand * A_i) arcs, its share of the
 * output arrays starts at the sum of the rooms before it.  out_nstates, out_narcs, status: device, per lattice;
 * states: the pair of every output state; arcs: per output arc its end points, the global word id, the input arc
 * (orig) and the two costs.  status: 0 ok, 2 the room is short (nothing is written outside
 * the lattice's share, its counts are 0), 3 empty or failed.  Null pointers, a non-finite scale, expand <= 0, a range
 * outside the batch, state_room / arc_room (elements) or work_bytes below what the range needs return PK2_ERR_INVALID
 * before the device is touched.  States of at most 64 candidate arcs are sorted by one wavefront, up to
 * PK2_LMRESCORE_SORT_LDS by the workgroup in LDS, above that in the workspace.
 * ------------------------------------------------------------------ */
#define PK2_NGRAM_MAX_ORDER 8
#define PK2_LMRESCORE_SORT_LDS 4096
typedef struct { int32_t s, h; } pk2_lm_state;                                   /* packed input state, LM node */
typedef struct { int32_t src, dst, word, orig; float graph, acoustic; } pk2_lm_arc;
int pk2_ngram_create(int32_t N, int32_t order, const int32_t* order_off, const int32_t* word, const float* cost,
                     const float* backoff, const int32_t* child_begin, const int32_t* bo_link, const int32_t* next_state,
                     int32_t start, int32_t eos, void* stream, void** out);
int pk2_ngram_destroy(void* h);
size_t pk2_wordlat_lmrescore_workspace_bytes(const void* h, int32_t first, int32_t count, double expand);
int pk2_wordlat_lmrescore(const void* h_lat, int32_t first, int32_t count, const void* h_lm, const int32_t* lm_word,
                          double scale, double expand, void* work, size_t work_bytes, int32_t* out_nstates,
                          int32_t* out_narcs, pk2_lm_state* states, size_t state_room, pk2_lm_arc* arcs, size_t arc_room,
                          int32_t* status, void* stream);

/* ------------------------------------------------------------------ *
 * Fused log-softmax + NLL + gradient. Replaces nn.CrossEntropyLoss
 * (ignore_index=-100; reduction mean: reference bin/train_ce.py:134,189;
 * reduction sum: bin/train_se.py:214,235).
 * loss_sum, count: device f32[1] / int32[1] accumulators (zeroed inside);
 * grad (optional) receives d(sum loss)/d logits, rows at grad_row_stride (rows
 * with ignore_index get zeros); the caller divides by count for the mean
 * reduction, or calls pk2_softmax_ce_fwd_bwd_mean.  A target outside
 * [0, num_classes) that is not ignore_index makes *loss_sum NaN, gets a zero
 * gradient row and is not counted.
 * logprob_out (optional, dense [rows][num_classes]) receives log softmax of
 * EVERY row, rows with an ignored or out-of-range target included.
 * ------------------------------------------------------------------ */
int pk2_softmax_ce_fwd_bwd(const float* logits, int64_t row_stride, const int64_t* targets,
                           int64_t ignore_index, int64_t rows, int32_t num_classes,
                           float* loss_sum, int32_t* count, float* grad, int64_t grad_row_stride,
                           float* logprob_out /* optional [rows][P] or NULL */, void* stream);
/* nn.CrossEntropyLoss(reduction='mean') in two launches with NO scaling pass over [rows, classes]: a one-workgroup launch
 * counts the valid targets into *count first, then the kernel above writes grad = d(mean loss)/d logits directly
 * (divided by max(1, count)); loss_sum stays the SUM of the row losses (reference bin/train_ce.py:134,189). */
int pk2_softmax_ce_fwd_bwd_mean(const float* logits, int64_t row_stride, const int64_t* targets,
                                int64_t ignore_index, int64_t rows, int32_t num_classes,
                                float* loss_sum, int32_t* count, float* grad, int64_t grad_row_stride, void* stream);
/* data[i] *= (*num_dev) / (*den_dev) IN PLACE (den_dev may be NULL = 1); when the factor is exactly 1 nothing is read or
 * written beyond the two scalars: the incoming gradient of loss.backward() (1.0) costs no pass over the gradient. */
int pk2_scale_inplace_ratio(float* data, int64_t n, const float* num_dev, const float* den_dev, void* stream);
/* grad *= (*scale_num) / max(1, *count_den) on the device (mean reduction). */
int pk2_scale_by_count(float* data, int64_t n, float numerator, const int32_t* count_den,
                       void* stream);
/* out[i] = in[i] * (*mul_dev) / max(1, *count_den_dev) in one pass (either pointer may be NULL = factor 1; out may equal in):
 * the gradient of nn.CrossEntropyLoss(reduction='mean') times the loss's incoming gradient, both factors on the device
 * (reference bin/train_ce.py:189-195: loss = criterion(...); loss.backward()). */
int pk2_scale_by_scalars(const float* in, float* out, int64_t n, const float* mul_dev, const int32_t* count_den_dev,
                         void* stream);

/* ------------------------------------------------------------------ *
 * f32 MFMA GEMM: C[M,N] (+)= alpha * op(A) * op(B) (+ bias[N]).
 * Replaces the cuBLAS calls under nn.Linear / nn.LSTM (reference
 * models/lstm.py:45-59).  Row-major; lda/ldb/ldc are row strides.
 * transa: A is stored [K,M];  transb: B is stored [N,K] (torch Linear weight).
 * ------------------------------------------------------------------ */
int pk2_gemm_f32(int32_t transa, int32_t transb, int32_t M, int32_t N, int32_t K, float alpha,
                 const float* A, int64_t lda, const float* B, int64_t ldb, float beta, float* C,
                 int64_t ldc, const float* bias, void* stream);
/* The product with the elementwise pass behind it in its epilogue: C = act(alpha op(A) op(B) + beta C + bias).
 * act 0: none (= pk2_gemm_f32); 1: ReLU (reference models/transformer.py:60, the encoder layer's
 * linear1 -> F.relu); 2: an element is kept where gate[m*ldg + n] > 0 and 0 elsewhere -- the ReLU's backward mask
 * read from the forward activation (what autograd's threshold_backward does behind the dX product).  Never cut
 * into atomically added K slices. */
int pk2_gemm_f32_act(int32_t transa, int32_t transb, int32_t M, int32_t N, int32_t K, float alpha,
                     const float* A, int64_t lda, const float* B, int64_t ldb, float beta, float* C,
                     int64_t ldc, const float* bias, int32_t act, const float* gate, int64_t ldg, void* stream);
/* Several products into one set of accumulators, one launch, fixed summation order:
 *   C = act(alpha * sum_{j < nseg} op(A + j*segA) * op(B + j*segB) + beta*C + bias),   K = depth of ONE segment.
 * TransformerAM's Conv1d(kernel 3, padding 1) over time (reference models/transformer.py:88-92: conv1d -> F.relu)
 * is nseg = 3 over row-shifted views of a zero-padded [B + T*B + B, C] activation buffer (segA = +-B*C floats,
 * segB = C*C: the taps' weight slices); segA / segB may be negative; transa = 0 only; act / gate as in
 * pk2_gemm_f32_act. */
int pk2_gemm_f32_seg(int32_t transa, int32_t transb, int32_t M, int32_t N, int32_t K, int32_t nseg, float alpha,
                     const float* A, int64_t lda, int64_t segA, const float* B, int64_t ldb, int64_t segB, float beta,
                     float* C, int64_t ldc, const float* bias, int32_t act, const float* gate, int64_t ldg,
                     void* stream);
/* Batched form: matrix triple z = i0*n1 + i1 (i0 < n0, i1 < n1) lives at offsets i0*stride?0 + i1*stride?1
 * (in floats) from A / B / C; no bias.  Used for the per-(utterance, head) attention products of
 * TransformerAM (reference models/transformer.py:60, nn.MultiheadAttention). */
int pk2_gemm_f32_batched(int32_t transa, int32_t transb, int32_t M, int32_t N, int32_t K, float alpha,
                         const float* A, int64_t lda, int64_t strideA0, int64_t strideA1, const float* B,
                         int64_t ldb, int64_t strideB0, int64_t strideB1, float beta, float* C, int64_t ldc,
                         int64_t strideC0, int64_t strideC1, int32_t n0, int32_t n1, void* stream);
/* Arithmetic of pk2_gemm_f32 / pk2_gemm_f32_batched (process-wide; default from PK2_GEMM_ARITH = bf16x3 | f32):
 *   0 = "f32":    v_mfma_f32_32x32x2_f32, bit-for-bit a k-ordered f32 fmaf chain (157 TFLOP/s peak) -- per K slice when
 *                 a deep product is cut into slices, which are added with float atomics
 *                 (tests/test_gpu_gemm.py::test_gemm_f32_against_fmaf_chain);
 *   1 = "bf16x3": every f32 operand element is split exactly into three bf16 numbers and six of the nine part products
 *                 run on v_mfma_f32_32x32x16_bf16 with f32 accumulation (csrc/gemm_bf16x3.h): error against float64 no
 *                 larger than the f32 product's -- measured rms 1.9-2.5e-8 of sum |a b| against 2.5-2.8e-8
 *                 (tests/test_gpu_gemm.py::test_gemm_error_bound_random_data), exact on integer-valued operands
 *                 (test_gemm_exact_families_poisoned) -- 2.67 x the matrix-core rate.  Same inputs, same outputs, same
 *                 memory traffic. */
int pk2_gemm_set_arith(int32_t arith);
int pk2_gemm_get_arith(void);
/* A Linear layer's weight AND bias gradient from one launch: C[M,N] = alpha * A^T B + beta * C with A stored [K,M] (= dY
 * [frames, out_features]), B [K,N] (= the layer's input), and colsum[m] += sum_k A[k][m] (the bias gradient, ACCUMULATED:
 * the buffer holds the gradient so far).  Replaces pk2_gemm_f32(1, 0, ...) followed by pk2_colsum_f32(A, ..., beta = 1). */
int pk2_gemm_f32_tn_colsum(int32_t M, int32_t N, int32_t K, float alpha, const float* A, int64_t lda, const float* B,
                           int64_t ldb, float beta, float* C, int64_t ldc, float* colsum, void* stream);
/* Row-mapped products: only the rows a map lists take part.  rmap is a device int32 array of Mv ASCENDING row indices of a
 * row-major matrix with M_total (K_total) rows -- for a time-major [T * B, .] minibatch the rows t * B + b with t < len_b, i.e.
 * the frames that are not padding.  Rows the map leaves out are neither read (they may hold anything, NaN included) nor
 * written.  rmap == NULL or Mv == the total row count is the unmapped entry, unchanged.
 *   pk2_gemm_f32_rows:            C[rmap[m], :] = alpha * A[rmap[m], :] * op(B) + beta * C[rmap[m], :] + bias,  m < Mv
 *                                 (A row-major [M_total, K]; transb as in pk2_gemm_f32; tiles / bands / K slices chosen for Mv rows)
 *   pk2_gemm_f32_tn_colsum_rows:  C = alpha * sum_{k<Kv} A[rmap[k], :]^T B[rmap[k], :] + beta * C,  colsum[m] += sum_{k<Kv} A[rmap[k]][m]
 *   pk2_rows_zero:                X[rows[i], 0..N) = 0, i < n  (the rows a mapped product did not write, without a fill of all of X)
 *   pk2_rows_pack:                out[i, 0..N) = X[rows[i], 0..N), i < n  (valid rows gathered into a dense matrix) */
int pk2_gemm_f32_rows(int32_t transb, int32_t M_total, int32_t N, int32_t K, float alpha, const float* A, int64_t lda,
                      const float* B, int64_t ldb, float beta, float* C, int64_t ldc, const float* bias,
                      const int32_t* rmap, int32_t Mv, void* stream);
int pk2_gemm_f32_tn_colsum_rows(int32_t M, int32_t N, int32_t K_total, float alpha, const float* A, int64_t lda, const float* B,
                                int64_t ldb, float beta, float* C, int64_t ldc, float* colsum, const int32_t* rmap, int32_t Kv,
                                void* stream);
int pk2_rows_zero(float* X, int64_t ldx, int32_t N, const int32_t* rows, int32_t n, void* stream);
int pk2_rows_pack(const float* X, int64_t ldx, int32_t N, const int32_t* rows, int32_t n, float* out, int64_t ldo, void* stream);
/* out[n] (+)= sum_m A[m][n]  (bias gradients). */
int pk2_colsum_f32(const float* A, int64_t lda, int32_t M, int32_t N, float beta, float* out,
                   void* stream);

/* ------------------------------------------------------------------ *
 * One (bi)directional LSTM layer, forward and backward through time.
 * Replaces the cuDNN RNN under nn.LSTM (reference models/lstm.py:49-58): gate
 * order i,f,g,o; h0 = c0 = 0; runs over all T frames of every sequence
 * (padding included, as the reference does).
 *
 * All activations are TIME-MAJOR (row = t*B + b) so that "previous step" is a
 * constant row offset and the W_hh gradient is one GEMM over shifted slices.
 * gx:  device f32 [T][B][D*4H], input projections x W_ih^T + b_ih of
 *      direction d at column offset d*4H (computed with pk2_gemm_f32).
 * whh: device f32 [D][4H][H] (weight_hh_l{k}, weight_hh_l{k}_reverse).
 * bhh: device f32 [D][4H] (bias_hh_l{k}[_reverse]) added inside, or NULL.
 * y:   device f32 [T][B][D*H] layer output (h_t; direction d at column d*H).
 * gates: device f32 [D][T][B][4H] post-activation i,f,g,o (saved for backward).
 * cells: device f32 [D][T][B][H] c_t (saved for backward).
 * H in {64,128,256,512,1024}.
 * ------------------------------------------------------------------ */
/* workspace: device f32, pk2_lstm_fwd_workspace_floats(B,H,D) floats (0 for small batches: may be NULL).
 * For B >= 32 the recurrence is tiled as a GEMM with W_hh rows regrouped per hidden unit in it. */
size_t pk2_lstm_fwd_workspace_floats(int32_t B, int32_t H, int32_t num_dirs);
int pk2_lstm_layer_fwd(const float* gx, const float* whh, const float* bhh, int32_t B, int32_t T,
                       int32_t H, int32_t num_dirs, float* y, float* gates, float* cells,
                       void* workspace, void* stream);
/* The same with the input projections computed inside the recurrence where the kernel can: inp (device f32
 * [T][B][in_size], the layer's input), w_ih (device f32 [D][4H][in_size]) and b_ih (device f32 [D][4H] or NULL) in place of
 * gx.  *gx_done = 1: the one-launch recurrence lstm_fwd_seq2_xproj multiplied on its idle MFMA pipe (H = 512, up to 8
 * (sequence, direction) pairs, in_size 80 or 1024, 16-byte aligned operands, a device whose first forward launch has been
 * verified); y, gates and cells are written and gx was not read (may be NULL).  *gx_done = 0: nothing was launched or
 * written; the caller computes gx with pk2_gemm_f32 and calls pk2_lstm_layer_fwd.  PK2_LSTM_SEQ_XPROJ (read per call):
 * 0 = never fused, 1 = the default, 2 = also 9 .. 32 pairs, queued behind one team per XCD. */
int pk2_lstm_layer_fwd_xproj(const float* gx, const float* whh, const float* bhh, int32_t B, int32_t T,
                             int32_t H, int32_t num_dirs, float* y, float* gates, float* cells, void* workspace,
                             const float* inp, int32_t in_size, const float* w_ih, const float* b_ih,
                             int32_t* gx_done, void* stream);
/* dy: device f32 [T][B][D*H] gradient wrt y.  dgx: device f32 [T][B][D*4H]
 * receives the gradient wrt the pre-activations (= gradient wrt gx).
 * scratch: device f32, at least pk2_lstm_bwd_scratch_floats(B,H,D). */
/* At H = 512 the whole recurrence of a layer runs in ONE persistent launch: lstm_fwd_seq2 / lstm_bwd_seq2 with a
 * (sequence, direction) pair per XCD for B*D <= 32 (csrc/lstm_persist_seq.hip; PK2_LSTM_SEQ=0 keeps the launch-per-step
 * kernels), lstm_fwd_big_persist / lstm_bwd_big_persist2 (lstm_bwd_big_persist for tensors that are not 16-byte aligned)
 * for B >= 32 (csrc/lstm_persist_big.hip; PK2_LSTM_BIG_PERSIST=0).
 * A poll of those kernels that times out leaves NaNs in the outputs and raises this flag (the call synchronises the
 * device). */
int pk2_lstm_persist_status(uint32_t* abort_flag);
/* Which kernels the most recent pk2_lstm_layer_fwd / pk2_lstm_layer_bwd[_bias] call of this process launched (host-side
 * bookkeeping, no synchronisation): the persistent paths fall back to the step kernels without an error (first-use check
 * failed, CU count, alignment, a backward call before a verified forward one), and this is how a caller or a test sees it.
 * STEP_SMALL: lstm_fwd_step / lstm_bwd_step_x4 (B < 32; the forward pass also for B >= 32 with a NULL workspace);
 * STEP_BIG: lstm_fwd_step_big / lstm_bwd_dh_big + lstm_bwd_pointwise_big; BIG_AG: the all-gather backward form. */
#define PK2_LSTM_PATH_NONE 0
#define PK2_LSTM_PATH_SEQ 1
#define PK2_LSTM_PATH_BIG 2
#define PK2_LSTM_PATH_BIG_AG 3
#define PK2_LSTM_PATH_STEP_SMALL 4
#define PK2_LSTM_PATH_STEP_BIG 5
int pk2_lstm_last_path(int32_t* fwd, int32_t* bwd);
size_t pk2_lstm_bwd_scratch_floats(int32_t B, int32_t H, int32_t num_dirs);
int pk2_lstm_layer_bwd(const float* dy, const float* whh, const float* gates, const float* cells,
                       int32_t B, int32_t T, int32_t H, int32_t num_dirs, float* dgx,
                       float* scratch, void* stream);
/* The same with the bias gradients where the kernel can produce them on the way: dbias_ih / dbias_hh (device f32
 * [D][4H], may be NULL) are ACCUMULATED into (+=; the caller zeroes them) with the sum over frames and sequences of dgx --
 * b_ih and b_hh of torch's LSTM receive the same gradient.  *bias_done = 1 when they were filled, 0 when the path taken
 * cannot (the caller then calls pk2_colsum_f32 on dgx). */
int pk2_lstm_layer_bwd_bias(const float* dy, const float* whh, const float* gates, const float* cells,
                            int32_t B, int32_t T, int32_t H, int32_t num_dirs, float* dgx, float* scratch,
                            float* dbias_ih, float* dbias_hh, int32_t* bias_done, void* stream);
/* The W_hh gradient dwhh[d] = sum_t dgates[d][t]^T h[d][t-1] (t+1 for the reverse direction)
 * is one pk2_gemm_f32 by the caller over row-shifted slices of dgx and y -- unless the recurrence has produced it on the
 * way: pk2_lstm_layer_bwd_wgrad is pk2_lstm_layer_bwd_bias plus y (device f32 [T][B][D*H], the forward pass's output,
 * before any dropout), dwhh (device f32 [D][4H][H], ACCUMULATED into, +=) and wgrad_ws (device f32, at least
 * pk2_lstm_bwd_wgrad_workspace_floats(B,H,D); may be NULL when that is 0).  *whh_done = 1 when dwhh has received the sum
 * (lstm_bwd_seq2_wgrad: each (sequence, direction) pair keeps its slice in MFMA accumulators, the sequences' slices are
 * added in ascending order, so repeated calls give the same bits; T = 1: nothing to add), 0 when the path taken left dwhh
 * and wgrad_ws untouched (every path but SEQ, a device on which the kernel's workgroups do not all fit, y not 16-byte
 * aligned, PK2_LSTM_SEQ_WGRAD=0 -- read per call).  A launch that gave up leaves NaNs in dwhh as in dgx -- and so does
 * every later *whh_done = 1 call on that stream, although its dgx is valid: the verdict read is the stream's sticky word
 * (what pk2_lstm_persist_status reports), which nothing clears, pk2_persist_guard_clear included.  A process that lowers
 * the guard and carries on sets PK2_LSTM_SEQ_WGRAD=0. */
size_t pk2_lstm_bwd_wgrad_workspace_floats(int32_t B, int32_t H, int32_t num_dirs);
int pk2_lstm_layer_bwd_wgrad(const float* dy, const float* whh, const float* gates, const float* cells, const float* y,
                             int32_t B, int32_t T, int32_t H, int32_t num_dirs, float* dgx, float* scratch,
                             float* dbias_ih, float* dbias_hh, float* dwhh, float* wgrad_ws, int32_t* bias_done,
                             int32_t* whh_done, void* stream);

/* ------------------------------------------------------------------ *
 * Row-wise pieces of TransformerAM (reference models/transformer.py:52-94: nn.TransformerEncoderLayer
 * post-norm + ReLU FFN, Conv1d(k=3)+ReLU per layer, final LayerNorm).
 * ------------------------------------------------------------------ */
/* s = x + res (res may be NULL); y = LayerNorm(s) * gamma + beta.  sum_out (may be NULL) receives s; mean,
 * rstd [rows] are saved for the backward pass. */
int pk2_layernorm_fwd(const float* x, const float* res, const float* gamma, const float* beta, int64_t rows,
                      int32_t C, float eps, float* sum_out, float* y, float* mean, float* rstd, void* stream);
/* ds = gradient wrt s; dgamma / dbeta are ACCUMULATED (+=). */
int pk2_layernorm_bwd(const float* dy, const float* s, const float* mean, const float* rstd,
                      const float* gamma, int64_t rows, int32_t C, float* ds, float* dgamma, float* dbeta,
                      void* stream);
/* scores [B*H][T][T] <- softmax over the last axis of (scores + src_mask[T][T]) with columns j where
 * key_padding[b][j] != 0 set to -inf, in place (src_mask / key_padding may be NULL). */
int pk2_softmax_mask_fwd(float* scores, const float* src_mask, const uint8_t* key_padding, int32_t B, int32_t H,
                         int32_t T, void* stream);
/* dP <- P * (dP - rowsum(dP * P)), in place. */
int pk2_softmax_bwd(const float* P, float* dP, int32_t BH, int32_t T, void* stream);

/* Fused multi-head self-attention (head size d = head_dim = 64 or 128): ctx = softmax(Q K^T * scale + src_mask, padded
 * keys -> -inf) V, read from / written to the packed time-major projections qkv[T*B][3*H*d] (row = t*B + b; Q | K | V,
 * head h at columns h*d) and ctx[T*B][H*d]; lse[B*H][T] = log-sum-exp of every score row, kept for the backward pass
 * (-inf, and ctx = 0, for a query with no visible key); dropout on the probabilities with the counter-based mask of
 * pk2_dropout_f32 indexed as a [B*H][T][T] matrix.  The scores never reach HBM.  Replaces the scaled-dot-product core of
 * nn.MultiheadAttention under nn.TransformerEncoderLayer (reference models/transformer.py:52-67).  Head size 64 is the
 * reference model's 512 / 8 (csrc/attention.hip), head size 128 the transformer command lines' default 512 / 4
 * (csrc/attention128.hip: one workgroup per CU); PK2_ERR_INVALID for other head sizes (callers keep the batched-GEMM form
 * for those). */
int pk2_attention_fwd(const float* qkv, int32_t T, int32_t B, int32_t H, int32_t head_dim, float scale,
                      const float* src_mask, const uint8_t* key_padding, float dropout_p, uint64_t seed, float* ctx,
                      float* lse, void* stream);
/* Gradient of the above by recomputation: dqkv[T*B][3*H*d] (every element written) from qkv, ctx, d ctx and lse;
 * dsum[B*H][T] is scratch (rowsum(dctx * ctx)).  Two launches: dQ (which also leaves dsum), then dK / dV (which reads it). */
int pk2_attention_bwd(const float* qkv, const float* ctx, const float* dctx, const float* lse, int32_t T, int32_t B,
                      int32_t H, int32_t head_dim, float scale, const float* src_mask, const uint8_t* key_padding,
                      float dropout_p, uint64_t seed, float* dqkv, float* dsum, void* stream);
/* One of the two launches of pk2_attention_bwd on its own, for timing tools (tools/attn_time.py): parts = 1: dQ and dsum,
 * 2: dK / dV from the dsum an earlier call left, 3: both = pk2_attention_bwd. */
int pk2_attention_bwd_part(int32_t parts, const float* qkv, const float* ctx, const float* dctx, const float* lse, int32_t T,
                           int32_t B, int32_t H, int32_t head_dim, float scale, const float* src_mask,
                           const uint8_t* key_padding, float dropout_p, uint64_t seed, float* dqkv, float* dsum, void* stream);
int pk2_relu_fwd(float* x, int64_t n, void* stream);                 /* in place */
int pk2_relu_bwd(const float* y, float* dy, int64_t n, void* stream); /* dy <- dy * (y > 0) */
int pk2_add_inplace(float* a, const float* b, int64_t n, void* stream);

/* Inverted dropout y = x * m/(1-p), m ~ Bernoulli(1-p), with a counter-based mask that is a pure
 * function of (seed, element index): calling it again on the gradient with the same seed applies the
 * same mask (no mask storage).  Replaces nn.LSTM's inter-layer dropout (reference models/lstm.py:49-54,
 * configs/ce.yaml:19).  x == y allowed. */
int pk2_dropout_f32(const float* x, float* y, int64_t n, float p, uint64_t seed, void* stream);

/* ------------------------------------------------------------------ *
 * Optimiser: global-norm clip + Adam(amsgrad) / SGD(momentum) over one flat
 * f32 parameter buffer.  Replaces clip_grad_norm_ + torch.optim.Adam / SGD
 * (reference bin/train_ce.py:123,195; bin/train_chain.py:138,287-288;
 * bin/train_se.py:127).
 * ------------------------------------------------------------------ */
/* norm_out: device f32[1] receives ||grad||_2. */
int pk2_grad_norm(const float* grad, int64_t n, float* norm_out, void* workspace,
                  size_t workspace_bytes, void* stream);
size_t pk2_grad_norm_workspace_bytes(int64_t n);
/* clip coefficient = min(1, max_norm / (*norm + 1e-6)) read on the device;
 * max_norm <= 0 disables clipping.  step is 1-based.  grad_scale multiplies the
 * gradient first (1/world_size for the averaged all-reduce).
 * beta1 / beta2 are float32 and the update is Adam with THOSE betas: 1 - beta and the bias corrections are formed
 * from them.  torch's float32 kernels use float32(0.999) for the decay but float32(1 - 0.999) for the new term;
 * 1 - float32(0.999) is 1.3e-5 below it, so exp_avg_sq (checkpointed state) is 1.3e-5 relative below torch's while
 * exp_avg_sq / (1 - beta2^t), and with it the parameters, agree. */
int pk2_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  float* max_exp_avg_sq /* NULL = no amsgrad */, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int64_t step, float max_norm,
                  const float* norm, float grad_scale, void* stream);
int pk2_sgd_step(float* param, const float* grad, float* momentum_buf /* NULL = none */,
                 int64_t n, float lr, float momentum, float weight_decay, int32_t first_step,
                 float max_norm, const float* norm, float grad_scale, void* stream);

/* ------------------------------------------------------------------ *
 * Guard of the persistent kernels (no reference counterpart: cuDNN / Kaldi kernels cannot time out).
 * The one-launch recurrences, the persistent denominator and the persistent lattice decoder poll each other's results
 * with a 1 s time-out; a launch that gave up has its output poisoned with NaN by a check kernel, which also raises this
 * per-device guard.  While it is raised pk2_adam_step / pk2_sgd_step leave parameters and moments untouched (so that a
 * poisoned gradient never reaches the weights, e.g. in bin/train_ce.py, which has no Kaldi-style NaN guard), and
 * pk2_persist_guard_status reports it WITHOUT synchronising (host-mapped word): pykaldi2_amd.optim raises at the next
 * step().  pk2_persist_guard_clear lowers it (synchronises); pk2_persist_guard_raise raises it from the device (tests).
 * ------------------------------------------------------------------ */
int pk2_persist_guard_status(uint32_t* raised);
int pk2_persist_guard_clear(void);
int pk2_persist_guard_raise(void* stream);
/* Several ranks (hvd.DistributedOptimizer, reference bin/train_chain.py:141-145): the guard is COLLECTIVE.  Before the
 * gradients are exchanged every rank exports its guard word into a one-float device slot, the slots are combined over the
 * ranks (pk2_allreduce_guarded below, or any max / sum all-reduce), and pk2_persist_guard_import raises the local guard
 * when any rank's was raised -- so no rank's optimiser kernel applies a gradient that holds a failed rank's NaN -- and
 * publishes the verdict of step `stamp` (1, 2, ...) in host-mapped memory.  pk2_persist_guard_verdict reads it without
 * synchronising; every rank reads the SAME verdict for the same stamp, so all ranks stop at the same step. */
int pk2_persist_guard_export(float* slot, void* stream);
int pk2_persist_guard_import(const float* slot, uint32_t stamp, void* stream);
int pk2_persist_guard_verdict(uint32_t stamp, uint32_t* ready, uint32_t* raised);

/* ------------------------------------------------------------------ *
 * Lattice path: on-the-fly lattice generation + lattice forward-backward for the MMI / sMBR / MPFE
 * criteria.  Replaces, for a whole minibatch and on the device, what MMIFunction / sMBRFunction do per
 * utterance on the CPU through PyKaldi (reference ops/ops.py:55-66, 133-146):
 *   asr_decoder.decode(loglikes)  [Kaldi LatticeFasterDecoder over HCLG, determinize_lattice = False,
 *                                  reference bin/train_se.py:172-183]
 *   scale_lattice + lattice_forward_backward_mmi(trans_model, lat, trans_ids, True, False, True)
 *   lattice_forward_backward_mpe_variants(trans_model, silence_phones, lat, trans_ids, criterion, True)
 *   Posterior.to_pdf_matrix(trans_model)
 * One workgroup per utterance; the lattices stay in the caller's workspace (device memory).
 * ------------------------------------------------------------------ */
typedef struct pk2_decode_graph pk2_decode_graph;

/* HCLG as arc arrays: ilabel = transition-id (0 = epsilon), weight = tropical cost, final_cost[s] = +inf for
 * non-final states.  Output labels (words) are not needed by any criterion and are not stored. */
int pk2_decode_graph_create(int32_t num_states, int32_t start_state, int64_t num_arcs,
                            const int32_t* arc_src, const int32_t* arc_dst, const int32_t* arc_ilabel,
                            const float* arc_weight, const float* final_cost, pk2_decode_graph** out);
/* HCLG.fst in OpenFst binary form ("vector" or "const" container, "standard" arcs;
 * reference bin/train_se.py:145,180). */
int pk2_decode_graph_from_openfst(const char* path, pk2_decode_graph** out);
/* The same with output labels (word ids; pk2_decode_graph_from_openfst keeps the olabels of the file), and the word of
 * the HCLG arc behind each link of an exported lattice (host arrays; -1 = no such arc): what the lattice-dumping command
 * line needs for `decoder_out["text"]` and the word labels of the compact lattice (reference bin/latgen.py:170-181). */
int pk2_decode_graph_create_words(int32_t num_states, int32_t start_state, int64_t num_arcs,
                                  const int32_t* arc_src, const int32_t* arc_dst, const int32_t* arc_ilabel,
                                  const int32_t* arc_olabel, const float* arc_weight, const float* final_cost,
                                  pk2_decode_graph** out);
int pk2_decode_graph_link_words(const pk2_decode_graph* g, int64_t num_links, const int32_t* src_state,
                                const int32_t* dst_state, const int32_t* tid, const float* graph_cost,
                                int32_t* word_out);
int pk2_decode_graph_destroy(pk2_decode_graph* g);
int pk2_decode_graph_info(const pk2_decode_graph* g, int32_t* num_states, int64_t* num_arcs,
                          int32_t* max_ilabel);

/* LatticeFasterDecoderOptions (reference bin/train_se.py:173-178; YAML decoder_config) + pool sizing. */
typedef struct {
  float beam;             /* 13 */
  float lattice_beam;     /* 7 */
  float beam_delta;       /* 0.5 */
  float acoustic_scale;   /* 0.1 */
  int32_t max_active;     /* 7000 */
  int32_t min_active;     /* 200 */
  int32_t tokens_per_frame;  /* pool size per utterance = (T+1) * this; 0 = max_active */
  int32_t links_per_frame;   /* pool size per utterance = (T+1) * this; 0 = 3 * max_active */
  /* (the Python wrapper passes 2 * max_active / 6 * max_active and quadruples them after an overflow report) */
} pk2_decoder_opts;

/* Layout of one minibatch of lattices (host object; lengths = frames per utterance). */
typedef struct pk2_lattice_batch pk2_lattice_batch;
int pk2_lattice_batch_create(const pk2_decode_graph* g, const int32_t* lengths_host, int32_t num_seq,
                             const pk2_decoder_opts* opts, pk2_lattice_batch** out);
size_t pk2_lattice_batch_bytes(const pk2_lattice_batch* b);
int pk2_lattice_batch_destroy(pk2_lattice_batch* b);

/* Decodes all utterances: loglikes[n][t][pdf] at n*seq_stride + t*frame_stride + pdf (device f32, the
 * acoustic model output minus the log prior, reference bin/train_se.py:241); tid2pdf: device i32
 * [num_tids + 1] (index 0 unused).  Asynchronous on `stream`; the lattices are left in `workspace`
 * (pk2_lattice_batch_bytes bytes, device). */
int pk2_lattice_decode(pk2_lattice_batch* b, const float* loglikes, int64_t seq_stride,
                       int64_t frame_stride, int32_t num_pdfs, const int32_t* tid2pdf, int32_t num_tids,
                       void* workspace, void* stream);
/* By default all frames of an utterance are decoded inside ONE persistent launch by a team of PK2_LAT_TEAM (8 / 16 / 32)
 * workgroups of one XCD (csrc/lattice_decode_frames.hip; PK2_LAT_DECODER=frames: a few launches per frame, =wg: one
 * workgroup per utterance).  *state: 1 = in use on this device, 0 = disabled or failed its first (host-verified) launch
 * -- the launch-per-frame decoder has taken over --, -1 = not tried yet; *abort_flag: some later launch timed out (its
 * utterances were reported with status 5, "not decoded").  Synchronises the device. */
int pk2_lattice_persist_status(int32_t* state, uint32_t* abort_flag);
/* Synchronises `stream` and reports per utterance: status (0 ok, 1 token pool overflow, 2 link pool
 * overflow, 3 no surviving token, 4 epsilon closure did not converge, 5 not decoded), tokens and links created, cost of
 * the best path.  Returns PK2_ERR_LIMIT / PK2_ERR_NUMERIC if any utterance failed.  Any output may be NULL. */
int pk2_lattice_summary(const pk2_lattice_batch* b, const void* workspace, int32_t* status,
                        int32_t* num_tokens, int32_t* num_links, float* best_cost, void* stream);
/* MMI: post[n][t][pdf] (+)= numerator - denominator posterior (lattice scaled by lm_scale / acoustic_scale
 * first, as fst::ScaleLattice does: float weights multiplied in double and stored back as float; 1.0 / 0.2
 * at reference ops/ops.py:58); frames whose reference transition-id is not in the lattice
 * are dropped when drop_frames != 0.  ref_tids: device i32, utterance n at n*ref_stride.  post rows must
 * be zero on entry.  lat_like: device f64[num_seq] = total log-likelihood of each lattice.
 * Any scale is allowed (so is any rescoring): the recursions (of mmi, mpe, posteriors and ts alike) keep a frame's values in
 * linear form, exp(value - the frame's log scale) in a double.  With the neighbouring frame's maximum scaled to 1 it holds a
 * token of a kept link down to 1e-280 (~645 nats) and a link whose scaled log-likelihood lies in [-708, 34.5].  A recursion
 * that meets anything beyond that -- a finished token value outside [1e-280, 1e200], a link weight outside [2.2e-308, 1e15] --
 * marks itself in the utterance's frame state and is run again in the log domain by the launch behind it (no host
 * synchronisation; utterances inside the range cost that launch a flag test): the results are those of a float64 log-domain
 * forward-backward over the whole range of the scores.  PK2_FB_LINEAR=0 (read once per process) runs everything in the log domain.
 * An utterance that failed to decode, or whose lattice has no path of non-zero weight (total likelihood not finite), gives
 * NaN here (and in pk2_lattice_mpe / pk2_lattice_posteriors) and nothing is added to its post rows. */
/* Which recursions of the last forward-backward call on the batch (mmi, mpe, posteriors; ts: its second one) left the linear
 * form's range and were run again in the log domain: rerun: device i32 [num_seq][2], [n][0] alpha, [n][1] beta; 1 = run again,
 * 0 = the linear kernel's values stood, -1 = no linear kernel ran (failed utterance, PK2_FB_LINEAR=0).  For tests and
 * diagnosis; the results do not depend on it.  Enqueued on `stream`. */
int pk2_lattice_fb_rerun(const pk2_lattice_batch* b, void* workspace, int32_t* rerun, void* stream);
int pk2_lattice_mmi(const pk2_lattice_batch* b, void* workspace, const int32_t* ref_tids,
                    int64_t ref_stride, const int32_t* tid2pdf, double lm_scale, double acoustic_scale,
                    int32_t drop_frames, float* post, int64_t post_seq_stride,
                    int64_t post_frame_stride, double* lat_like, void* stream);
/* sMBR (criterion 0) / MPFE (criterion 1): post (+)= arc posterior * (expected accuracy through the arc -
 * expected accuracy); score: device f64[num_seq] = expected frame accuracy.  tid2phone: device i32
 * [num_tids + 1]; phone_is_silence: device u8 [num_phones + 1]. */
int pk2_lattice_mpe(const pk2_lattice_batch* b, void* workspace, const int32_t* ref_tids,
                    int64_t ref_stride, const int32_t* tid2pdf, const int32_t* tid2phone,
                    const uint8_t* phone_is_silence, int32_t criterion, int32_t one_silence_class,
                    double lm_scale, double acoustic_scale, float* post, int64_t post_seq_stride,
                    int64_t post_frame_stride, double* score, void* stream);
/* N-best paths of the decoded lattices (reference nbest_as_fsts on convert_lattice_to_std of the lattice scaled by
 * lattice_scale(lm_scale, acoustic_scale)).  `scratch`: device memory of pk2_lattice_nbest_bytes() bytes for the same
 * (num_paths, total_tokens, total_links, distinct, label_cap); total_tokens / total_links = sums of pk2_lattice_summary's
 * num_tokens / num_links.  label_mode 0 = HCLG output labels (words; the graph needs them), 1 = phones through
 * tid2label (device i32 [num_tids + 1]: phone of a transition-id of HMM state 0 that is not a self-loop, else 0).
 * distinct != 0: the num_paths best distinct label sequences.  Outputs (device): num_hyp [N] = M; hyp_path [N][num_paths]
 * = path of hypothesis m (reference mode drops paths that repeat an earlier path's labels); per path cost [N][num_paths],
 * label count path_nlab (-1: more than label_cap labels), labels [N][num_paths][label_cap], transition-ids
 * [N][num_paths][Tmax].  num_paths must be in 1..64. */
size_t pk2_lattice_nbest_bytes(const pk2_lattice_batch* b, int32_t num_paths, int64_t total_tokens, int64_t total_links,
                               int32_t distinct, int32_t label_cap);
int pk2_lattice_nbest(const pk2_lattice_batch* b, void* workspace, void* scratch, int64_t total_tokens,
                      int64_t total_links, int32_t num_paths, int32_t distinct, int32_t label_mode,
                      const int32_t* tid2label, int32_t num_tids, double lm_scale, double acoustic_scale,
                      int32_t label_cap, int32_t* num_hyp, int32_t* hyp_path, float* path_cost, int32_t* path_nlab,
                      int32_t* path_labels, int32_t* path_tids, void* stream);
/* N-best minimum word error (reference MWEFunction): the N-best of pk2_lattice_nbest, e_k = Levenshtein distance of
 * hypothesis k to the supervision (device i32 [N][sup_stride], sup_len [N], at most 1023 labels), p_k = 1/M
 * (equal_weight) or softmax(-cost), loss [N] f64 = sum e_k p_k; grad (zero-filled by the caller) [n, t, tid2pdf[tid_k[t]]]
 * = sum of (e_k - loss) p_k.  A failed utterance gives NaN and no gradient. */
int pk2_lattice_mwe(const pk2_lattice_batch* b, void* workspace, void* scratch, int64_t total_tokens,
                    int64_t total_links, int32_t num_paths, int32_t distinct, int32_t label_mode,
                    const int32_t* tid2label, int32_t num_tids, double lm_scale, double acoustic_scale,
                    int32_t label_cap, int32_t equal_weight, const int32_t* sup, int64_t sup_stride,
                    const int32_t* sup_len, const int32_t* tid2pdf, int32_t num_pdfs, float* grad,
                    int64_t grad_seq_stride, int64_t grad_frame_stride, double* loss, void* stream);
/* Kaldi's RescoreLattice on the decoded lattices, in place: the acoustic cost of every kept emitting link t -> t+1 with
 * transition-id tid becomes  float(float(old_acoustic_scale * cost) - loglikes[n][t][tid2pdf[tid]])  (old_acoustic_scale 0:
 * exactly -loglike; 1: the new score is added to the old one, as RescoreLattice does; Kaldi's discriminative trainers scale
 * the old scores by 0 first).  loglikes is addressed as in pk2_lattice_decode (any model's output for the same frames;
 * num_pdfs must be the decode's).  Epsilon links, tokens, graph and final costs, segments and the pruning result are not
 * touched: pk2_lattice_summary's best_cost and the exported token costs stay those of the decode.  Every later call on the
 * batch (mmi, mpe, nbest, mwe, posteriors, export) sees the rescored lattice. */
int pk2_lattice_rescore(const pk2_lattice_batch* b, void* workspace, const float* loglikes, int64_t seq_stride,
                        int64_t frame_stride, int32_t num_pdfs, const int32_t* tid2pdf, int32_t num_tids,
                        float old_acoustic_scale, void* stream);
/* Kaldi's LatticeForwardBackward + Posterior.to_pdf_matrix with no reference alignment: post[n][t][pdf] += post_sign *
 * (sum of the posteriors of the frame's links with that pdf) on the lattice scaled by lm_scale / acoustic_scale as in
 * pk2_lattice_mmi; lat_like: device f64[num_seq] = total log-likelihood (NaN for a failed utterance and for a lattice without
 * a path of non-zero weight, which adds nothing to post). */
int pk2_lattice_posteriors(const pk2_lattice_batch* b, void* workspace, const int32_t* tid2pdf, double lm_scale,
                           double acoustic_scale, float post_sign, float* post, int64_t post_seq_stride,
                           int64_t post_frame_stride, double* lat_like, void* stream);
/* Lattice teacher-student step (the intent of reference ops/ops.py:77-117) in one launch chain: forward-backward on the
 * lattice as decoded from the teacher (like_T, gamma_T), pk2_lattice_rescore with the student's loglikes_S, forward-backward
 * again (like_S, gamma_S).  loss [N] f64 = sum_l gamma_T(l) (like_T(l) - like_S(l)) - like_T + like_S = KL(P_T || P_S) over the
 * lattice's paths; grad (zero-filled by the caller) [n][t][pdf] = gamma_S - gamma_T summed per pdf = d loss / d loglikes_S
 * divided by acoustic_scale.  loss, like_T, like_S: device f64[num_seq].  The batch is left rescored.  An utterance whose
 * rescored lattice has no path of non-zero weight gives loss NaN and a zero gradient. */
int pk2_lattice_ts(const pk2_lattice_batch* b, void* workspace, const float* loglikes_S, int64_t seq_stride,
                   int64_t frame_stride, int32_t num_pdfs, const int32_t* tid2pdf, int32_t num_tids,
                   float old_acoustic_scale, double lm_scale, double acoustic_scale, float* grad,
                   int64_t grad_seq_stride, int64_t grad_frame_stride, double* loss, double* like_T, double* like_S,
                   void* stream);
/* Test / tooling hook: copies the pruned lattice of utterance n to host arrays (synchronises `stream`).
 * Call with null arrays to get the counts.  Tokens are renumbered frame by frame; link_ac is the acoustic
 * cost with the acoustic scale removed. */
int pk2_lattice_export(const pk2_lattice_batch* b, const void* workspace, int32_t n, int32_t* num_tokens,
                       int32_t* num_links, int32_t* tok_frame, int32_t* tok_state, float* tok_cost,
                       float* tok_final, int32_t* link_src, int32_t* link_dst, int32_t* link_tid,
                       float* link_graph, float* link_ac, void* stream);

/* Lattice determinisation on word labels (host arrays in, host handle out; no device work).  Replaces, for the lattice
 * dump of reference bin/latgen.py:143-181, what PyKaldi's recogniser does when `determinize_lattice = True`
 * (bin/latgen.py:149: Kaldi's DeterminizeLatticePhonePrunedWrapper): the result accepts every word sequence of the raw
 * state-level lattice once, with the (graph, acoustic) costs and the transition-id alignment of its best path
 * (CompactLattice semantics, no minimisation).  Arc i of the input: src[i] -> dst[i], word[i] (0 = epsilon), tid[i] (0 =
 * none), costs graph[i], acoustic[i]; final_cost[s] (+inf = not final).  beam: what lies on no complete path within beam
 * of the best one is dropped, before and after the subset construction (pass the decoder's lattice beam); more than
 * max_states output states -> PK2_ERR_LIMIT (retry with a smaller beam, as Kaldi's wrapper does). */
typedef struct pk2_det_lattice pk2_det_lattice;
int pk2_lattice_determinize(int32_t num_states, int32_t start, int64_t num_arcs, const int32_t* src, const int32_t* dst,
                            const int32_t* word, const int32_t* tid, const float* graph, const float* acoustic,
                            const float* final_cost, double beam, int64_t max_states, pk2_det_lattice** out);
int pk2_det_lattice_sizes(const pk2_det_lattice* h, int32_t* num_states, int32_t* start, int64_t* num_arcs,
                          int64_t* arc_tids, int64_t* final_tids);
/* Arcs sorted by (source state, word): src, dst, word, graph, acoustic [num_arcs], tid_off [num_arcs + 1] into tids;
 * per state final_graph / final_acoustic (+inf = not final) and final_tid_off [num_states + 1] into final_tids. */
int pk2_det_lattice_export(const pk2_det_lattice* h, int32_t* src, int32_t* dst, int32_t* word, float* graph,
                           float* acoustic, int64_t* tid_off, int32_t* tids, float* final_graph, float* final_acoustic,
                           int64_t* final_tid_off, int32_t* final_tids);
void pk2_det_lattice_destroy(pk2_det_lattice* h);

/* ------------------------------------------------------------------------------------------------
 * Gradient exchange: RCCL all-reduce over xGMI, one communicator per process (= per GPU).
 * Replaces horovod.torch's NCCL all-reduce hidden in hvd.DistributedOptimizer.step()
 * (reference bin/train_chain.py:141-145, bin/train_ce.py:127-131, bin/train_se.py:130-134).
 * librccl is bound at run time (dlopen; a copy already mapped into the process is reused; PK2_RCCL_LIB
 * overrides).  Only the unique id travels through the launcher's own channel (torch.distributed store /
 * broadcast in pykaldi2_amd/hvd.py, MPI in the reference).
 * ---------------------------------------------------------------------------------------------- */
typedef struct pk2_comm pk2_comm;
/* Size of a unique id in bytes (NCCL_UNIQUE_ID_BYTES = 128). */
int32_t pk2_comm_unique_id_bytes(void);
/* Rank 0: generates the id every rank must pass to pk2_comm_init (host buffer of pk2_comm_unique_id_bytes()). */
int pk2_comm_unique_id(void* id_out);
/* Collective over all ranks (ncclCommInitRank on the calling thread's current device). */
int pk2_comm_init(int32_t rank, int32_t world, const void* unique_id, pk2_comm** out);
/* In-place SUM all-reduce of buf[0..count) (device f32: a bucket of the flat gradient buffer) enqueued on `stream`
 * (hipStream_t): the compute stream, or a side stream the caller fences with events.  Averaging (1/world) is folded
 * into the optimiser kernel (pk2_adam_step / pk2_sgd_step grad_scale), not done here. */
int pk2_allreduce_bucket(pk2_comm* comm, float* buf, int64_t count, void* stream);
/* The same plus, in the same RCCL group (one launch), the max over the ranks of the one-float guard slot
 * (pk2_persist_guard_export / _import above). */
int pk2_allreduce_guarded(pk2_comm* comm, float* buf, int64_t count, float* guard_slot, void* stream);
/* rank / world of the communicator and the path of the RCCL library in use (any output may be NULL). */
int pk2_comm_info(const pk2_comm* comm, int32_t* rank, int32_t* world, char* lib_path, int32_t lib_path_bytes);
int pk2_comm_destroy(pk2_comm* comm);

/* ------------------------------------------------------------------------------------------------
 * Side streams confined to a part of the chip (no reference counterpart: cuBLAS / cuDNN own the whole GPU).  The weight
 * gradients of a layer hang off the serial chain of the backward pass (reference models/lstm.py:49-58 through autograd);
 * pykaldi2_amd.lstm can launch them on a side stream (PK2_SIDE_STREAM=1), and with PK2_SIDE_CU_PER_XCD=k that stream is
 * created with a CU mask: the first k CUs of every XCD (hipExtStreamCreateWithCUMask; mask bit i = CU i / 8 of XCD i % 8 on
 * this 8-XCD part -- pk2_debug_where reports where the workgroups of a launch really ran).
 * ---------------------------------------------------------------------------------------------- */
int pk2_stream_create_cu_mask(int32_t cus_per_xcd, void** stream_out);
int pk2_stream_destroy(void* stream);
/* out[3 * b + {0, 1, 2}] = XCC id, shader engine, CU of workgroup b of a `blocks`-workgroup launch on `stream` (HW_ID). */
int pk2_debug_where(int32_t* out, int32_t blocks, void* stream);
/* Stand-in for the collective library's all-reduce kernel on a one-GPU box (PK2_HVD_FAKE_PEER in pykaldi2_amd/hvd.py):
 * `blocks` workgroups stream dst[i] += src[i] over n floats, `passes` times, on `stream`. */
int pk2_debug_peer_reduce(float* dst, const float* src, int64_t n, int32_t blocks, int32_t passes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PK2HIP_H_ */
