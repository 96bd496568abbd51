// qv_match_wide.hip -- the matching kernels (qv_match_body.inc) for the opt-in window of 2,048 normalised characters
// (qv_config.max_transcript = QV_MAX_TRANSCRIPT_WIDE): 32-word transcript patterns, 2 KB code rows, 10 KB mask tables per
// pattern.  The kernels land in namespace qv_wide (distinct names in profiles and disassembly).
#define QV_MAXQ QV_MAX_TRANSCRIPT_WIDE
#define QV_MATCH_NS qv_wide
#define QV_MATCH_SET qv_match_wide
#include "qv_match_body.inc"
