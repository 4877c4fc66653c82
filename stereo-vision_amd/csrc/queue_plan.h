// Queue plan of the ELAS engine: which HIP streams a lane owns, in which stream priority class each of them is
// created, and which of them every phase of a group runs on.  Pure arithmetic -- no HIP call, no environment access --
// so that the table can be checked on the CPU (tests/cxx/queue_plan_check.cpp, tests/test_queue_plan.py).
//
// Why classes: the HIP runtime multiplexes the streams of a process onto at most GPU_MAX_HW_QUEUES hardware queues
// (default 4) PER STREAM PRIORITY CLASS (low, normal, high), and kernels of one hardware queue run one after the
// other.  A host program that started the runtime before svh_init could ask for more queues leaves the 12 lane
// streams of six workers on 4 queues; streams of another class draw from a pool of their own.  See DESIGN.md,
// "Queue plans".
#ifndef SVH_QUEUE_PLAN_H
#define SVH_QUEUE_PLAN_H

#include <stdlib.h>

namespace svh {

enum { QC_NORMAL = 0, QC_HIGH = 1, QC_LOW = 2, QC_COUNT = 3 };        // stream priority classes
enum { QPH_A = 0, QPH_S = 1, QPH_B = 2, QPH_COUNT = 3 };              // phases: Sobel + support, stage chain, planes .. mean
enum { QP_AUTO = -1, QP_ONE = 0, QP_STAGE_HIGH = 1, QP_SECOND_LOW = 2, QP_BY_PHASE = 3, QP_PARITY = 4, QP_LAST = 4 };
// Plans 1-3 split a group over streams of its lane, linked with events.  QP_PARITY keeps every group on ONE stream and
// spreads whole lanes over two classes instead: the single stream of every worker's second lane is in the low class.
// It is the only layout that measured faster than QP_ONE; 1-3 are kept for repeating the A/B on another runtime or part.

constexpr int kQueueCapDefault = 4;   // the runtime's own GPU_MAX_HW_QUEUES when the variable is unset
constexpr int kQueueBudget = 12;      // hardware queues the engine may hold in one process
// The plan automatic mode takes where the cap is below the number of lane streams: the one layout that separated
// from QP_ONE in the A/B on the device ("Queue plans": the table; profiles/queue_plan_ab.txt).
constexpr int kQueuePlanWhenShort = QP_PARITY;

// the streams of one lane: stream 0 is the main stream (the one the lane's waits and copies use)
struct QueueLane {
    int nstreams;                // 1..3
    int cls[QC_COUNT];           // class of stream k, k < nstreams
    int phase_stream[QPH_COUNT]; // stream of phase A, S, B
};
struct QueuePlan {
    int plan;                    // the plan in effect (a request may degrade: see make_queue_plan)
    QueueLane lane[2];           // by lane parity: first / second lane of a worker
    int streams_per_lane;        // the larger of the two
    int classes;                 // distinct classes over both parities
    int queues;                  // hardware queues `workers` workers hold with it: per class min(cap, streams)
};

// GPU_MAX_HW_QUEUES as the runtime reads it: unset, empty or not a positive number = 4
inline int queue_cap_from_text(const char* text) {
    if (!text || !*text) return kQueueCapDefault;
    const long v = strtol(text, nullptr, 10);
    if (v <= 0) return kQueueCapDefault;
    return v > 1024 ? 1024 : (int)v;
}

// the class a wanted class becomes under the device's priority range [greatest, least] (numerically greatest <=
// least; hipDeviceGetStreamPriorityRange): normal is 0 clamped into the range, high / low exist when the range
// reaches beyond normal on their side, a missing class folds into normal
inline int queue_priority_normal(int least, int greatest) { return 0 < greatest ? greatest : (0 > least ? least : 0); }
inline int queue_fold_class(int cls, int least, int greatest) {
    const int normal = queue_priority_normal(least, greatest);
    if (cls == QC_HIGH && greatest < normal) return QC_HIGH;
    if (cls == QC_LOW && least > normal) return QC_LOW;
    return QC_NORMAL;
}
// the priority value a stream of class `cls` (already folded) is created with
inline int queue_priority_of(int cls, int least, int greatest) {
    return cls == QC_HIGH ? greatest : cls == QC_LOW ? least : queue_priority_normal(least, greatest);
}

// classes of the three phases under `plan` for lane parity `parity`, before folding
inline void queue_plan_wanted(int plan, int parity, int out[QPH_COUNT]) {
    out[QPH_A] = out[QPH_S] = out[QPH_B] = QC_NORMAL;
    if (plan == QP_STAGE_HIGH || plan == QP_SECOND_LOW) out[QPH_S] = QC_HIGH;
    if ((plan == QP_SECOND_LOW || plan == QP_PARITY) && parity == 1) out[QPH_A] = out[QPH_B] = QC_LOW;   // the main stream of every worker's second lane
    if (plan == QP_PARITY && parity == 1) out[QPH_S] = QC_LOW;   // (the whole group: one stream)
    if (plan == QP_BY_PHASE) {
        out[QPH_S] = QC_HIGH;
        out[QPH_B] = QC_LOW;
    }
}

inline QueuePlan queue_plan_layout(int least, int greatest, int cap, int workers, int plan) {
    QueuePlan q{};
    q.plan = plan;
    int per_class[QC_COUNT] = {0, 0, 0};
    for (int parity = 0; parity < 2; parity++) {
        QueueLane& L = q.lane[parity];
        int want[QPH_COUNT];
        queue_plan_wanted(plan, parity, want);
        // one stream per class the lane's phases use; phase A's class gets stream 0
        for (int ph = 0; ph < QPH_COUNT; ph++) {
            const int c = queue_fold_class(want[ph], least, greatest);
            int k = 0;
            while (k < L.nstreams && L.cls[k] != c) k++;
            if (k == L.nstreams) L.cls[L.nstreams++] = c;
            L.phase_stream[ph] = k;
        }
        for (int k = 0; k < L.nstreams; k++) per_class[L.cls[k]] += workers;
        if (L.nstreams > q.streams_per_lane) q.streams_per_lane = L.nstreams;
    }
    for (int c = 0; c < QC_COUNT; c++)
        if (per_class[c]) {
            q.classes++;
            q.queues += per_class[c] < cap ? per_class[c] : cap;
        }
    return q;
}

// The plan for a device whose priority range is [greatest, least], at a queue cap of `cap` per class, for `workers`
// double-buffered workers.  requested: QP_AUTO or 0..QP_LAST.
//   * QP_AUTO: kQueuePlanWhenShort where the cap is below the number of lane streams (2 x workers), else QP_ONE
//     (the host program already provides a queue per lane stream).
//   * A plan whose layout would hold more than kQueueBudget hardware queues degrades to QP_ONE (plan 1 at a cap of 8
//     and six workers: 8 normal + 8 high).
//   * Missing priority levels fold into normal; phases of one class share one stream, so a one-level range gives
//     the one-stream layout whatever was asked.
inline QueuePlan make_queue_plan(int least, int greatest, int cap, int workers, int requested) {
    if (least < greatest) { const int t = least; least = greatest; greatest = t; }
    if (cap < 1) cap = 1;
    if (workers < 1) workers = 1;
    int plan = requested;
    if (plan < 0 || plan > QP_LAST) plan = cap < 2 * workers ? kQueuePlanWhenShort : QP_ONE;
    QueuePlan q = queue_plan_layout(least, greatest, cap, workers, plan);
    if (plan != QP_ONE && q.queues > kQueueBudget) q = queue_plan_layout(least, greatest, cap, workers, QP_ONE);
    if (q.streams_per_lane == 1 && q.classes == 1) q.plan = QP_ONE;   // everything folded: it IS the one-stream layout
    return q;
}

}  // namespace svh
#endif
