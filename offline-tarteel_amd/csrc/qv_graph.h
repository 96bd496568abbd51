// qv_graph.h -- a run of launches captured into one hipGraph (the forward, the post-logits chain) and the forward's cache policy.
#pragma once

#include "qv_common.h"
#include "qv_graph_policy.h"

// Captures what `launch` enqueues on `s` (thread-local capture) and instantiates it: *captured = true and *exec is ready to
// launch.  Any failure of the capture machinery (a capture-unsafe call of the host on this thread invalidated it, a node type
// the runtime cannot instantiate) must not fail the batch -- the plain launches would have succeeded: the sticky error is
// cleared, *captured = false, QV_OK, and the caller switches graphs off for its context and issues the launches for real.
// `launch`'s own error code comes back as it is and is no capture failure.
template <typename Fn>
int qv_capture_graph(hipStream_t s, Fn &&launch, hipGraphExec_t *exec, bool *captured) {
    *exec = nullptr;
    *captured = false;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        hipGraph_t graph = nullptr;
        const int rc = launch();
        hipError_t e = hipStreamEndCapture(s, &graph);
        if (!rc && e == hipSuccess) e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
        if (graph) (void)hipGraphDestroy(graph);
        if (rc) return rc;
        *captured = e == hipSuccess && *exec;
    }
    if (!*captured) { (void)hipGetLastError(); *exec = nullptr; }
    return QV_OK;
}
