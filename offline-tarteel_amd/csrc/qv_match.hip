// qv_match.hip -- the matching kernels (qv_match_body.inc) for the default window of 1,024 normalised characters.
#define QV_MAXQ QV_MAX_TRANSCRIPT
#define QV_MATCH_NS   // anonymous namespace
#define QV_MATCH_SET qv_match_default
#include "qv_match_body.inc"
