// What a training step hands from launcher to launcher, as structs (host only: none of these is a kernel argument).
// The extern "C" entry points keep their positional lists and pack them; loc_train_step builds each struct once.
#pragma once
#include "stack_tail.h"

// the minibatch: n_b row indices into the genotype matrix
struct step_rows { const uint8_t* X; int64_t x_pitch; const int32_t* rows; int n_b; };

// layer 1's trainable state with its Adam moments, in the order of the entry points' parameter lists
struct l1_state { float *w1s, *m1s, *v1s, *gamma, *beta, *m_gamma, *v_gamma, *m_beta, *v_beta, *b1, *m_b1, *v_b1; };
static inline l1_state l1_state_of(float* P, float* M, float* V, const loc_layout& lay) {
    return {P + lay.w1,    M + lay.w1,   V + lay.w1,   P + lay.gamma, P + lay.beta, M + lay.gamma,
            V + lay.gamma, M + lay.beta, V + lay.beta, P + lay.b1,    M + lay.b1,   V + lay.b1};
}

// what adam_alpha() reads: the step-size table, the learning rate and the step count t_base + t_off
struct adam_clock { const float* alpha_tab; int alpha_tab_len; const float* lr; const int* t_base; int t_off; };
static inline adam_clock adam_clock_of(const loc_net* net, int t_off) {
    return {net->alpha_tab, net->alpha_tab_len, net->lr, net->t_base, t_off};
}

// the kernel argument of the row-reducing tail (stack_tail.h), filled in its field order; the six offsets are loc_layout's
// wh, bh, wa, ba, wb, bb
static inline loc_dw_tail_args dw_tail_args_of(int L, int n_pre, int n_b, int slot_rows, int use_drop, const float* acts,
                                               const float* adrop, const float* dz, const float* head_out, float* P,
                                               float* M, float* V, float* WhT, int64_t off_wh, int64_t off_bh,
                                               int64_t off_wa, int64_t off_ba, int64_t off_wb, int64_t off_bb,
                                               float* loss_out, const adam_clock& c) {
    return {L, n_pre, n_b, use_drop, acts, adrop, dz, head_out, P, M, V, WhT, off_wh, off_bh, off_wa, off_ba, off_wb, off_bb,
            loss_out, c.alpha_tab, c.alpha_tab_len, c.lr, c.t_base, c.t_off, slot_rows};
}

// stack_fused.hip: the entry point of this name on a filled argument block (gb may be NULL: no gamma / beta blocks)
int loc_stack_dw_adam_tail(int Hp, const loc_dw_tail_args& ta, const loc_gb_tail* gb, void* stream);

// the gamma / beta update behind the layer-1 backward's main kernel: the next step's statistics (or NULL), where its scale /
// shift go, and an event to record between the two launches (or NULL)
struct l1_gb_stage { const float* bn_next_stats; float* bn4_out; void* ev_after_main; };
// l1_kernels.hip: loc_l1_backward_adam (in_mask NULL) / _in_dropout.  gb NULL: the main kernel (W1 / b1) only, like
// loc_l1_backward_adam_main; the caller then runs the gamma / beta update that consumes gb_scratch
int l1_backward_impl(const step_rows& r, const loc_dims* d, const float* bn4, const float* dz1, const l1_state& s,
                     float* gb_scratch, const adam_clock& c, int grid, const loc_tuning* tune, const uint8_t* in_mask,
                     float in_ks, const l1_gb_stage* gb, void* stream);

// l1_chain.hip: loc_l1_backward_adam_chain with the tail above as trailing workgroups of the same launch (tail may be NULL)
int l1_chain_launch(const step_rows& r, const int32_t* rows_next, int n_b_next, const loc_dims* d, float* bn4,
                    const float* bn_next_stats, const float* dz1, const l1_state& s, const adam_clock& c, int grid,
                    float* partial, int64_t partial_floats, const loc_tuning* tune, const loc_dw_tail_args* tail, int rb,
                    void* stream);
