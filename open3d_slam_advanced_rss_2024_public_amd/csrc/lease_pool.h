// lease_pool.h — the process-wide pool behind every leased work area (the pinned landing areas of cloud_dev.h, the registration
// areas of o3d_icp_impl.h, the RANSAC areas of ransac_impl.h).  Standard library only.
//
// Areas are expensive to make (device and pinned allocations stall the device for milliseconds), so a call takes an idle one of
// its key (the device index), or a fresh T when there is none, and gives it back when it is done.  The pool is leaked on purpose:
// it is never destroyed, because the destructors of its areas call into the HIP runtime, and a static destructor can run after
// the runtime has been unloaded (exit-time crashes).  Areas die only through drop_idle().
#pragma once
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

namespace o3s {

template <typename T>
class LeasePool {
 public:
  static LeasePool& get() {
    static LeasePool* pool = new LeasePool;  // leaked deliberately (see above)
    return *pool;
  }
  // an idle area given under `key` (the one that has been idle longest), or a fresh T
  std::unique_ptr<T> take(int key) {
    {
      std::lock_guard<std::mutex> g(m_);
      for (size_t k = 0; k < idle_.size(); ++k)
        if (idle_[k].first == key) {
          std::unique_ptr<T> a = std::move(idle_[k].second);
          idle_.erase(idle_.begin() + (long)k);
          return a;
        }
    }
    return std::unique_ptr<T>(new T);
  }
  void give(int key, std::unique_ptr<T> a) {
    if (!a) return;
    std::lock_guard<std::mutex> g(m_);
    idle_.emplace_back(key, std::move(a));
  }
  // destroys the idle areas of `key`; areas of other keys and areas out on a lease are left alone
  void drop_idle(int key) {
    std::vector<std::unique_ptr<T>> gone;  // destroyed after the lock is released
    std::lock_guard<std::mutex> g(m_);
    for (size_t k = 0; k < idle_.size();)
      if (idle_[k].first == key) {
        gone.push_back(std::move(idle_[k].second));
        idle_.erase(idle_.begin() + (long)k);
      } else {
        ++k;
      }
  }

 private:
  LeasePool() = default;
  std::mutex m_;
  std::vector<std::pair<int, std::unique_ptr<T>>> idle_;
};

}  // namespace o3s
