// Who counts on which chain-counter area of a workspace, and whether that area is still zero: decided here and nowhere else
// (DESIGN.md section 24).  Host code only.
#pragma once
#include "gru_chain.h"

constexpr long kSyncBlockWords = (long)kSyncAreas * kChainSyncWords;    // a workspace's sync block: what a carve takes, what a call zeroes at once

// What a chain launch is given: GruChainFwd / GruChainBwd / DecodeChainArgs ::counters and ::prezeroed are these two values, nothing else.
struct SyncArea { unsigned* counters; int prezeroed; };

// One ledger per library call and sync block: one clean bit per area.  The call tells it when it has zeroed the whole block (its prologue
// launch, or its hipMemsetAsync); every launch site asks it for the area it counts on (the modules' area maps name them: vae.hip next to
// dec_carve, seq.hip next to bigru2_carve).  An area is handed out as `prezeroed` while its bit is set, and handing it out clears the bit: the
// launch counts it up, so whoever takes it next has its launcher zero it first.
// A clean bit holds for the call's stream and for streams forked from it AFTER the zeroing (twin_fork / side_fork inside gru_layer_fwd and
// bigru2_core_fwd, which all come behind the prologue or the memset): a launch on any other stream must not take an area from this ledger.
// It holds for one call.  The one promise that crosses calls has its own entry, carried_over().
struct SyncLedger {
    explicit SyncLedger(unsigned* block = nullptr) : base(block) {}
    void zeroed_all() { clean = (1u << kSyncAreas) - 1; }
    // `area` is still zero from the block-wide zeroing of an EARLIER call on the same stream, which took other areas only (stage 2 of the
    // staged encoder backward, behind stage 1: bigru2_core_bwd)
    void carried_over(int area) { if (area >= 0 && area < kSyncAreas) clean |= 1u << area; }
    // 0 and *out, or -1 for an area outside the block (or no block): never a pointer then
    int take(int area, SyncArea* out) {
        if (!base || area < 0 || area >= kSyncAreas) return -1;
        const unsigned bit = 1u << area;
        out->counters = base + (long)area * kChainSyncWords;
        out->prezeroed = (clean & bit) != 0;
        clean &= ~bit;
        used |= bit;
        self_zeroed += !out->prezeroed;
        return 0;
    }
    unsigned* base;
    unsigned clean = 0;
    unsigned used = 0;                            // areas handed out so far (a dry run reads and may reset it: vae.hip dec_route_areas)
    int self_zeroed = 0;                          // launches so far whose launcher zeroes their area
};
