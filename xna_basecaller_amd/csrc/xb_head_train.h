// xb_head_train.h -- what xb_head.hip's trainer shares with the trainer of the top layers (xb_top.hip): the check that a
// context's head runs in three fp16 products, the gradient's norm, AdamW and its scalars, and the tail of a step.  Unless said
// otherwise: no argument checks, launches on the context's main stream, no synchronisation.  Private to csrc/; include after
// xb_ctx.h.
#pragma once

int head_usable(xb_ctx *ctx, const char *who);
// *d_norm = (float)sqrt(sum a^2 + sum b^2) in float64, xb_grad_norm_dev's order
int grad_norm_run(xb_ctx *ctx, const float *d_a, size_t na, const float *d_b, size_t nb, float *d_norm);
int adamw_run(xb_ctx *ctx, float *p, float *g, float *m, float *v, size_t len, float clip, float decay, float step_size, float bc2_sqrt);
// decay, step_size and bc2_sqrt of step `step` (1, 2, ..) at learning rate lr, in double, rounded once
void adamw_scalars(double lr, long step, float *decay, float *step_size, float *bc2_sqrt);

// The tail of a trainer's step, in the three parts a call `who` runs around its own gradient.
// 1. After the call's own "is a trainer open": a context ready for n chunks, no null argument, with `step` a learning rate that is
//    finite and not negative, the label batch (label_batch_check), then `enter`.
int train_call_enter(xb_ctx *ctx, const char *who, const float *signal, int n, const uint8_t *targets, int Lt, const int32_t *lengths,
                     bool step, float lr, const float *loss, const float *grad_norm);
// 2. Behind the gradient: the norm and the n chunks' losses back on the host, synchronised; the mean is taken in double.
int train_read_back(xb_ctx *ctx, const float *d_norm, const float *d_loss, int n, float *norm, float *mean_loss);
// 3. The clipped update of step `step` (1, 2, ..) over `len` floats of p, g, m, v: a norm that is not finite is refused with the
//    weights unchanged; else clip_grad_norm_(max_norm = 2.0)'s factor, AdamW's scalars, one launch.  The one place that knows
//    the clipping policy.
int train_update(xb_ctx *ctx, const char *who, float norm, float lr, long step, float *p, float *g, float *m, float *v, size_t len);
