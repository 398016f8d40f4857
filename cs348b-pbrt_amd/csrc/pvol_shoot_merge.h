// pvol_shoot_merge.h -- the merge of PhotonShootingTask::Run (core/photonshooter.cpp:280-351) as a pure object: the bookkeeping of
// the shoot and one round's decisions from the round's count table.  Plain C++, no HIP: pvol_shoot_host.hip drives the device with
// what round() returns, tests/test_shoot_merge.py replays tables through it (pvol_shoot_merge_replay) without a GPU.
#ifndef PVOL_SHOOT_MERGE_H
#define PVOL_SHOOT_MERGE_H
#include <algorithm>
#include <vector>
#include "../../include/pvol.h"

// The rows of one store: who appended which rows where.  Segments are in global order; localRows[r] counts rank r's rows so far.
struct __attribute__((visibility("hidden"))) Plan {
    std::vector<uint32_t> src, local, global;
    std::vector<uint64_t> localRows;
    uint64_t rows = 0;
    void add(uint32_t r, uint32_t n) {
        if (!n) return;
        src.push_back(r); local.push_back((uint32_t)localRows[r]); global.push_back((uint32_t)rows);
        localRows[r] += n; rows += n;
    }
    uint64_t most() const { uint64_t m = 0; for (uint64_t v : localRows) m = std::max(m, v); return m; }
};

// One rank's own appends of a round, by slot: volume {slot, count, local offset, float(running nshot)} and surface
// {slot, nSurf, take, nRad, off[4] = caustic, direct, indirect, radiance}
struct __attribute__((visibility("hidden"))) ShootAppends {
    std::vector<uint32_t> vTask, vCount, vOff, sTask, sN, sTake, sRad, sOff;
    std::vector<float> vNshot;
};

struct __attribute__((visibility("hidden"))) ShootMerge {
    const uint32_t T, R, blockPaths;
    const bool keep;
    const uint32_t wantCaustic, wantIndirect, wantVolume;
    std::vector<uint32_t> flags;   // [T] bit0 causticDone, bit1 indirectDone, bit2 volumeDone, bit3 finished
    uint32_t nshot = 0;
    uint64_t nVolume = 0, nCaustic = 0, nDirect = 0, nIndirect = 0, nRadTotal = 0;
    uint32_t nCausticPaths = 0, nDirectPaths = 0, nIndirectPaths = 0;
    bool abortTasks = false;
    uint32_t stallRounds = 0;   // rounds in a row without a photon for a store still wanted
    int status = PVOL_OK;   // or PVOL_E_SHOOT_FAILED
    Plan plan[5];   // volume, caustic, direct, indirect, radiance
    ShootAppends mine;

    ShootMerge(uint32_t nTasks, uint32_t nRanks, uint32_t blockPaths_, bool keep_, uint32_t nCausticWanted, uint32_t nIndirectWanted, uint32_t nVolumeWanted)
        : T(nTasks), R(nRanks), blockPaths(blockPaths_), keep(keep_), wantCaustic(nCausticWanted), wantIndirect(nIndirectWanted), wantVolume(nVolumeWanted),
          flags(nTasks, (nCausticWanted == 0 ? 1u : 0u) | (nIndirectWanted == 0 ? 2u : 0u) | (nVolumeWanted == 0 ? 4u : 0u)) {
        for (Plan &p : plan) p.localRows.assign(R, 0);
    }
    size_t rowWords() const { return 1 + 8 * (size_t)((T + R - 1) / R); }
    bool anyLive() const { for (uint32_t f : flags) if (!(f & 8u)) return true; return false; }
    static bool unsuccessful(uint32_t needed, uint64_t found, uint32_t shot) { return (found < needed && (found == 0 || found < shot / 1024)); }   // photonshooter.cpp:37-39
    void giveUp() { nVolume = 0; nCaustic = nIndirect = 0; nRadTotal = 0; abortTasks = true; status = PVOL_E_SHOOT_FAILED; }   // :292-298 erases caustic, indirect, volume, radiance

    // Merges one round in task order.  `table` is the exchanged one, rank-major: rowWords() words a rank, word 0 its status, then 8
    // words a slot, task t in slot t / R of rank t % R.  Returns `rank`'s own appends; none in a round that gave up (the stores
    // are erased, their plans are never used, and the next anyLive() finds every task finished).
    const ShootAppends &round(const uint32_t *table, uint32_t rank) {
        mine = ShootAppends();
        const uint64_t volBefore = nVolume, causticBefore = nCaustic, indirectBefore = nIndirect;
        for (uint32_t t = 0; t < T; ++t) {
            uint32_t &fl = flags[t];
            if (fl & 8u) continue;
            if (abortTasks) { fl |= 8u; continue; }
            // photonshooter.cpp:283-290; 4096 is the reference's constant in this test, whatever the block
            if (nshot > 500000 && (unsuccessful(wantCaustic, nCaustic, 4096) || unsuccessful(wantIndirect, nIndirect, 4096) || unsuccessful(wantVolume, nVolume, 4096))) {
                giveUp(); fl |= 8u; continue;
            }
            nshot += blockPaths;
            const uint32_t owner = t % R, slot = t / R;
            const uint32_t *lc = &table[owner * rowWords() + 1 + 8 * (size_t)slot];
            uint32_t take = 0;
            if (!(fl & 2u)) {
                take |= 2u | 4u;
                nIndirectPaths += blockPaths; nDirectPaths += blockPaths;
                nIndirect += lc[3];
                if (nIndirect >= wantIndirect) fl |= 2u;
                nDirect += lc[2];
            }
            if (!(fl & 1u)) {
                take |= 1u;
                nCausticPaths += blockPaths;
                nCaustic += lc[1];
                if (nCaustic >= wantCaustic) fl |= 1u;
            }
            if (keep && (lc[4] || lc[5])) {
                // kind k's records of the block number lc[1 + k]; they go to store k only when bit k of `take` is set
                const uint32_t n[4] = {(take & 1u) ? lc[1] : 0u, (take & 2u) ? lc[2] : 0u, (take & 4u) ? lc[3] : 0u, lc[5]};
                if (owner == rank) {
                    mine.sTask.push_back(slot); mine.sN.push_back(lc[4]); mine.sTake.push_back(take); mine.sRad.push_back(lc[5]);
                    for (int k = 0; k < 4; ++k) mine.sOff.push_back((uint32_t)plan[1 + k].localRows[rank]);
                }
                for (int k = 0; k < 4; ++k) plan[1 + k].add(owner, n[k]);
            }
            nRadTotal += keep ? lc[5] : 0;
            if (!(fl & 4u)) {
                if (lc[0]) {
                    if (owner == rank) {
                        mine.vTask.push_back(slot); mine.vCount.push_back(lc[0]); mine.vOff.push_back((uint32_t)plan[0].localRows[rank]);
                        mine.vNshot.push_back(float(nshot));
                    }
                    plan[0].add(owner, lc[0]);
                    nVolume += lc[0];
                }
                if (nVolume >= wantVolume) fl |= 4u;
            }
            if ((fl & 7u) == 7u) fl |= 8u;
        }
        if (abortTasks) return mine = ShootAppends();
        // The reference has no exit for a store that stops growing after a good start (`unsuccessful` passes once found >= 4): e.g. a
        // matte scene whose "caustic" photons all come through the medium, after the volume map is full -- it would shoot forever.  Here 256
        // rounds in a row without a photon for any store still wanted end the pass the way the reference's own abort does, on the global counts.
        const bool progress = nCaustic != causticBefore || nIndirect != indirectBefore || nVolume != volBefore;
        stallRounds = progress ? 0u : stallRounds + 1u;
        if (stallRounds >= 256u) { giveUp(); for (uint32_t &f : flags) f |= 8u; }
        return mine;
    }
};
#endif
