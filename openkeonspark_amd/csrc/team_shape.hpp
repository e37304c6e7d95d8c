// The ONE host-side rule that maps an embedding width D to a team shape (L, C): L lanes own one row, each lane holds C
// elements (team.hpp).  Every launch site picks its kernel instantiation through these helpers, so two kernels that must
// agree bit for bit on a width (emit / apply, the inverse-norm pre-pass / apply, kge_transe_record_dwords / emit) cannot
// land on different rungs.  A rung with C too small would not fault: the `e < D` guard silently drops the tail elements.
#pragma once
#include "../../include/kge_mi355.h"

namespace kge {

template <int L_, int C_>
struct TeamShape {
    static constexpr int L = L_, C = C_;
};

// Plain ladder.  Calls f(TeamShape<L, C>{}) once for the rung of width D and returns true; false = no shape (D > 1024).
template <class F>
inline bool for_team_shape(int D, F &&f) {
    if (D <= 16) f(TeamShape<16, 1>{});
    else if (D <= 32) f(TeamShape<16, 2>{});
    else if (D <= 64) f(TeamShape<16, 4>{});
    else if (D <= 128) f(TeamShape<32, 4>{});
    else if (D <= 256) f(TeamShape<64, 4>{});
    else if (D <= 512) f(TeamShape<64, 8>{});
    else if (D <= 1024) f(TeamShape<64, 16>{});
    else return false;
    return true;
}

// TransE count-path ladder: a width that is a multiple of 4 up to 64 takes the vectorised (16, 4) kernels (one float4 per
// lane), every other width the plain rung.
template <class F>
inline bool for_transe_team_shape(int D, F &&f) {
    if (D % 4 == 0 && D <= 64) { f(TeamShape<16, 4>{}); return true; }
    return for_team_shape(D, f);
}

// For the entry points that have never refused a width: beyond the ladder they keep taking its last rung (whose `e < D` guard
// drops the elements past 1024).  Existing behaviour, held in this one place; a new site refuses instead.
template <class F>
inline void for_team_shape_or_last(int D, F &&f) {
    if (!for_team_shape(D, f)) f(TeamShape<64, 16>{});
}
template <class F>
inline void for_transe_team_shape_or_last(int D, F &&f) {
    if (!for_transe_team_shape(D, f)) f(TeamShape<64, 16>{});
}

template <int MODEL_>
struct ModelTag {
    static constexpr int MODEL = MODEL_;
};

// The same for the model id, for the sites that accept all four models: f(ModelTag<MODEL>{}); false = unknown model id.
template <class F>
inline bool for_model(int model, F &&f) {
    switch (model) {
        case KGE_TRANSE: f(ModelTag<KGE_TRANSE>{}); return true;
        case KGE_TRANSH: f(ModelTag<KGE_TRANSH>{}); return true;
        case KGE_TRANSR: f(ModelTag<KGE_TRANSR>{}); return true;
        case KGE_TRANSD: f(ModelTag<KGE_TRANSD>{}); return true;
        default: return false;
    }
}

}  // namespace kge
