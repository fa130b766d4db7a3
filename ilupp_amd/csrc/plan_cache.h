// ilupp_amd/csrc/plan_cache.h -- parked analysis plans, by shape: what destroy_obj keeps of a box-grid ILU(0) object's dimension-derived
// tables for the next object of the same shape (api.hip).  A host-only class template, free of HIP like pool.h, so that it can be
// exercised on the CPU under AddressSanitizer (tests/test_plan_cache_host.py builds tests/plan_cache_harness.cpp).
//
// Rules:
//   * a plan is MOVED in (park) and MOVED out (take): it has one owner at any time -- the object it was built for, the cache, or the
//     object that adopted it.  Nothing is shared, nothing is counted;
//   * the cache knows a plan as a key, a payload it never looks into, and a list of opaque blocks with their sizes; a plan that leaves the
//     cache other than through take() -- evicted, dropped, refused -- has `release` called exactly once on every one of its blocks;
//   * at most `capacity` plans per device, the least recently parked one leaves first; one plan per key (a second one of a key that is
//     parked already is refused: the parked one is as good, and becomes the most recent);
//   * park() is told how many bytes the cache may hold after it (the caller's byte limit minus what else it counts against it): a plan
//     that does not fit is refused, parked plans are not evicted for bytes -- shrink_to() does that when the limit itself falls;
//   * its own mutex: parking happens from destroy calls, which hold no other lock.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <list>
#include <mutex>
#include <utility>
#include <vector>

namespace ilupp {

struct PlanKey {
    int device = 0;
    int32_t n = 0;
    int64_t nnz = 0;
    int32_t nx = 0, ny = 0, nz = 0;
    bool operator==(const PlanKey &o) const { return device == o.device && n == o.n && nnz == o.nnz && nx == o.nx && ny == o.ny && nz == o.nz; }
};

struct PlanBlock { void *handle; size_t bytes; };

template <class Payload>
class PlanCache {
public:
    typedef void (*Release)(void *handle);
    struct Plan {
        PlanKey key;
        Payload payload;
        std::vector<PlanBlock> blocks;
        size_t bytes() const { size_t b = 0; for (const PlanBlock &k : blocks) b += k.bytes; return b; }
    };
    // what ilupp_hip_plan_cache_stats hands out: plans parked now, plans taken, takes that found none, plans that left unadopted
    struct Stats { unsigned long long parked, taken, missed, dropped; };

    PlanCache(Release release, size_t capacity_per_device) : release_(release), cap_(capacity_per_device ? capacity_per_device : 1) {}
    ~PlanCache() { drop_all(); }
    PlanCache(const PlanCache &) = delete;
    PlanCache &operator=(const PlanCache &) = delete;

    // the plan goes in (true) or its blocks are released (false: its key is parked already, or it holds more than `room` bytes together
    // with what is parked).  A device's plan beyond the capacity leaves, the least recently parked first.
    bool park(Plan &&plan, size_t room)
    {
        std::vector<PlanBlock> out;
        bool parked = false;
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto same = plans_.end();
            for (auto it = plans_.begin(); it != plans_.end(); ++it) if (it->key == plan.key) same = it;
            const size_t b = plan.bytes();
            if (same != plans_.end()) {
                plans_.splice(plans_.end(), plans_, same);
                out.swap(plan.blocks);
            } else if (b > room || bytes_ > room - b) {
                out.swap(plan.blocks);
            } else {
                bytes_ += b; blocks_ += plan.blocks.size();
                const int dev = plan.key.device;
                plans_.push_back(std::move(plan));
                parked = true;
                size_t on_dev = 0;
                for (const Plan &p : plans_) if (p.key.device == dev) ++on_dev;
                for (auto it = plans_.begin(); on_dev > cap_ && it != plans_.end();) {
                    if (it->key.device != dev) { ++it; continue; }
                    it = unlink(it, &out);
                    --on_dev;
                }
            }
        }
        release_all(out);
        return parked;
    }

    // the plan of that key comes out (true; it is the caller's now) or none is parked (false)
    bool take(const PlanKey &key, Plan *out)
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (auto it = plans_.begin(); it != plans_.end(); ++it) {
            if (!(it->key == key)) continue;
            bytes_ -= it->bytes(); blocks_ -= it->blocks.size();
            *out = std::move(*it);
            plans_.erase(it);
            ++taken_;
            return true;
        }
        ++missed_;
        return false;
    }

    // every plan leaves
    void drop_all() { shrink_to(0, true); }

    // the least recently parked plans leave until no more than `room` bytes are parked (everything: every plan, whatever it weighs)
    void shrink_to(size_t room, bool everything = false)
    {
        std::vector<PlanBlock> out;
        {
            std::lock_guard<std::mutex> lk(mu_);
            while (!plans_.empty() && (everything || bytes_ > room)) unlink(plans_.begin(), &out);
        }
        release_all(out);
    }

    // a plan that was taken and then did not serve (the matrix was not of its shape): its new owner has released it
    void note_dropped() { std::lock_guard<std::mutex> lk(mu_); ++dropped_; }

    size_t bytes() const { std::lock_guard<std::mutex> lk(mu_); return bytes_; }
    size_t blocks() const { std::lock_guard<std::mutex> lk(mu_); return blocks_; }
    size_t plans() const { std::lock_guard<std::mutex> lk(mu_); return plans_.size(); }
    Stats stats() const
    {
        std::lock_guard<std::mutex> lk(mu_);
        return Stats{(unsigned long long)plans_.size(), taken_, missed_, dropped_};
    }

private:
    typedef typename std::list<Plan>::iterator It;
    It unlink(It it, std::vector<PlanBlock> *out)              // (lock held)
    {
        bytes_ -= it->bytes(); blocks_ -= it->blocks.size();
        out->insert(out->end(), it->blocks.begin(), it->blocks.end());
        ++dropped_;
        return plans_.erase(it);
    }
    void release_all(const std::vector<PlanBlock> &v) { for (const PlanBlock &k : v) release_(k.handle); }     // (outside the lock: it may take the pool's)

    Release release_;
    size_t cap_;
    mutable std::mutex mu_;
    std::list<Plan> plans_;                                    // the least recently parked first
    size_t bytes_ = 0, blocks_ = 0;
    unsigned long long taken_ = 0, missed_ = 0, dropped_ = 0;
};

}  // namespace ilupp
