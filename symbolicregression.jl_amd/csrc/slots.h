// slots.h — the slot registry of a context (host only): the stable column
// number of every shared subtree (jit.h Columns::gkey) that the context's
// programs have asked for. Tree code bakes the column number into its address
// arithmetic, so a subtree that keeps its number from program to program can
// be read from a column another program left in the dataset's pool (api.cpp
// srhip_dataset::pool) instead of being derived again.
//
// The registry only hands out numbers. What a slot of a dataset's pool holds
// is recorded with the pool and compared key by key before every launch, so
// a displaced key is derived again by its owner's next call and correctness
// never depends on the registry's history.
#pragma once
#include <algorithm>
#include <cstdint>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

namespace srhip {

class SlotRegistry {
 public:
  explicit SlotRegistry(int nslot = 64) : key_((size_t)(nslot > 0 ? nslot : 0)), used_(key_.size(), 0) {}
  int nslot() const { return (int)key_.size(); }
  // The slots of one program's keys (distinct), all below `limit`: a key the
  // registry holds keeps its slot; a new one takes the lowest free slot or
  // else displaces the least recently used key that this program does not
  // use itself. False (nothing changed): more keys than slots below `limit`.
  bool assign(const std::vector<std::string>& keys, int limit, std::vector<int>* slots) {
    std::lock_guard<std::mutex> lk(mu_);
    const int n = std::min(limit, nslot());
    if ((int)keys.size() > n) return false;
    slots->assign(keys.size(), -1);
    std::vector<char> mine((size_t)std::max(n, 0), 0);
    // a held key above the limit (a program with more LDS columns) moves below it
    for (size_t k = 0; k < keys.size(); ++k) {
      auto it = slot_.find(keys[k]);
      if (it == slot_.end() || it->second >= n) continue;
      (*slots)[k] = it->second;
      mine[(size_t)it->second] = 1;
    }
    ++clock_;
    for (size_t k = 0; k < keys.size(); ++k) {
      int s = (*slots)[k];
      if (s < 0) {
        for (int j = 0; j < n; ++j) {  // free first, else the oldest that is not this program's
          if (mine[(size_t)j]) continue;
          if (key_[(size_t)j].empty()) { s = j; break; }
          if (s < 0 || used_[(size_t)j] < used_[(size_t)s]) s = j;
        }
        if (!key_[(size_t)s].empty()) slot_.erase(key_[(size_t)s]);
        auto old = slot_.find(keys[k]);  // (held above the limit)
        if (old != slot_.end()) {
          key_[(size_t)old->second].clear();
          slot_.erase(old);
        }
        key_[(size_t)s] = keys[k];
        slot_[keys[k]] = s;
        mine[(size_t)s] = 1;
        (*slots)[k] = s;
      }
      used_[(size_t)s] = clock_;
    }
    return true;
  }
  // the key a slot was last given to ("": never used)
  std::string key(int slot) const {
    std::lock_guard<std::mutex> lk(mu_);
    return slot >= 0 && slot < nslot() ? key_[(size_t)slot] : std::string();
  }

 private:
  mutable std::mutex mu_;
  std::vector<std::string> key_;
  std::vector<uint64_t> used_;
  std::unordered_map<std::string, int> slot_;
  uint64_t clock_ = 0;
};

}  // namespace srhip
