// A few most-recently-used results keyed by the numbers they were computed from: what a plan keeps of the data-independent
// geometry of a bin set (cells and mean separation per bin, modes per (k, mu) cell, sorted row lists), so that a repeated
// call with the same edges skips the pass that computes it.  Standard C++ only.
#pragma once
#include <cstddef>
#include <list>
#include <utility>
#include <vector>

template <typename V, size_t CAP> class FbKeyedCache {
    std::list<std::pair<std::vector<double>, V>> e_;       // most recent last
public:
    // the value stored under `key`, which becomes the most recent entry, or null; valid until the entry is evicted
    V* find(const std::vector<double>& key) {
        for (auto it = e_.begin(); it != e_.end(); ++it)
            if (it->first == key) {
                e_.splice(e_.end(), e_, it);
                return &it->second;
            }
        return nullptr;
    }
    // stores `value` under a key that find() has just missed; with CAP entries held, the least recently used one is destroyed
    V* insert(std::vector<double> key, V value) {
        if (e_.size() >= CAP) e_.pop_front();
        e_.emplace_back(std::move(key), std::move(value));
        return &e_.back().second;
    }
};
