// qv_limits.h -- plain constants shared by the kernels and by the HIP-free host code (qv_tables_host.h,
// qv_weights_host.h): the alphabet, the span and verse-text limits, the model's dimensions.  Nothing but <stdint.h> and
// the public header behind it.
#pragma once

#include <stdint.h>

#include "../../include/qverse.h"   // QV_VOCAB, the error codes

#define QV_NSYM 40          // alphabet codes 0..39 (0 = ' '); 63 = matches nothing
#define QV_OTHER 63
#define QV_MAX_SPAN 6
#define QV_MAX_VW 11        // ceil(684 / 64): words of the longest verse text

// Frames of one utterance: qv_create refuses an engine whose frame capacity (t_cap: the frames of max_samples, + 2) is above
// QV_MAX_T_CAP, and the per-frame arrays the greedy kernels keep in LDS (k_decode, k_transcribe) hold QV_FRAME_CAP entries.
#define QV_MAX_T_CAP 768
#define QV_FRAME_CAP 770
static_assert(QV_FRAME_CAP >= QV_MAX_T_CAP, "the LDS frame arrays hold the frames of the largest engine");

// FastConformer-CTC dimensions
#define QV_D 512
#define QV_H 8
#define QV_DK 64
#define QV_FF 2048
#define QV_NMEL 80
#define QV_SUBC 256
#define QV_N_LAYERS 17

// launch-shape constants the kernels (qv_frontend.hip, qv_attention.hip) and the host's launch plans (qv_launch_plan.h) share
#define SUB_TT 4            // k_sub01: c1 frames per tile
#define SUB_MAX_RUN 16      // k_sub01: tiles a block walks at most
#define SUB_RES_RUN 4       // k_sub01: tiles a block walks at most with the run's mel rows resident in LDS
#define S35_TC 3            // k_sub35: c2 frames per step
#define S35_MAX_RUN 16      // k_sub35: steps a block walks at most
#define ATT_SHORT_T 128     // longest utterance (encoder frames) k_attention_short takes

#ifdef __HIPCC__
#define QV_HOST_DEVICE __host__ __device__
#else
#define QV_HOST_DEVICE
#endif

// word counts the LCS core is instantiated for; verse match-mask rows are padded to these
QV_HOST_DEVICE inline int qv_tmpl_w(int w) {
    return w <= 1 ? 1 : w <= 2 ? 2 : w <= 3 ? 3 : w <= 4 ? 4 : w <= 6 ? 6 : w <= 8 ? 8 : w <= 11 ? 11 : 16;
}
