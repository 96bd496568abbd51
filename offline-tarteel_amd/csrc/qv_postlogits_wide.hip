// qv_postlogits_wide.hip -- the post-logits kernels and launchers once more, for the opt-in matching window of 2,048
// normalised characters (qv_config.max_transcript = QV_MAX_TRANSCRIPT_WIDE): 32-word transcript patterns, 2 KB code rows,
// 10 KB mask tables per pattern.  The source is qv_postlogits.hip; the kernels land in namespace qv_wide (distinct names in
// profiles and disassembly), the launchers get the suffix _wide, and qv_capi.hip picks a set per engine (QV_POST).
#define QV_MAXQ 2048
#include "qv_common.h"
static_assert(QV_MAXQ == QV_MAX_TRANSCRIPT_WIDE, "the wide kernel set is built for QV_MAX_TRANSCRIPT_WIDE");

namespace qv_wide {}
using namespace qv_wide;
#define QV_POST_NS qv_wide
#define qv_post_run qv_post_run_wide
#define qv_post_debug_retrieve qv_post_debug_retrieve_wide
#define qv_post_tracker_match qv_post_tracker_match_wide
#define qv_post_match_verse qv_post_match_verse_wide

#include "qv_postlogits.hip"
