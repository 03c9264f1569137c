// kbhip session, part 09: the prologue the task queries share (session.h: query_task, query_begin)
#include "session.h"

namespace kbhip {

const HPod& query_task(const Session& S, int pod, const string& prefix, bool need_job, const char* no_class_prefix) {
    if (pod < 0 || pod >= (int)S.pods.size() || S.pods[pod].cls < 0)
        throw Error(KBHIP_EINVAL, (no_class_prefix ? string(no_class_prefix) : prefix) +
                                      "has no task class (not a pending task of the session)");
    const HPod& p = S.pods[pod];
    if (p.status != Pending) throw Error(KBHIP_EINVAL, prefix + "is not Pending (the session placed it)");
    if (need_job && (p.job < 0 || S.jobs[p.job].queue < 0 || S.jobs[p.job].queue >= (int)S.queues.size()))
        throw Error(KBHIP_EINVAL, prefix + "has no job");
    return p;
}

void query_begin(Session& S, const char* api_name) {
    if (S.world != 1) throw Error(KBHIP_EUNSUPPORTED, string(api_name) + " on a node-sharded session");
    ov_quiesce(S);
}

}  // namespace kbhip
