// xb_head_train.h -- what xb_head.hip's trainer shares with the trainer of the top layers (xb_top.hip): the check that a
// context's head runs in three fp16 products, the gradient's norm, AdamW and its scalars.  No argument checks, launches on the
// context's main stream, no synchronisation.  Private to csrc/; include after xb_ctx.h.
#pragma once

int head_usable(xb_ctx *ctx, const char *who);
// *d_norm = (float)sqrt(sum a^2 + sum b^2) in float64, xb_grad_norm_dev's order
int grad_norm_run(xb_ctx *ctx, const float *d_a, size_t na, const float *d_b, size_t nb, float *d_norm);
int adamw_run(xb_ctx *ctx, float *p, float *g, float *m, float *v, size_t len, float clip, float decay, float step_size, float bc2_sqrt);
// decay, step_size and bc2_sqrt of step `step` (1, 2, ..) at learning rate lr, in double, rounded once
void adamw_scalars(double lr, long step, float *decay, float *step_size, float *bc2_sqrt);
