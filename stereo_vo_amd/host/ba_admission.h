// The admission ledger of kernels whose workgroups wait for each other (the wide device-resident solve, csrc/ba.hip
// ba_fused_budget), free of the GPU: plain POSIX plus atomics.  One BaLedger per device of a process counts the workgroups the
// process has admitted there, and — the budget belongs to the GPU, not to a process — mirrors that count into a table shared
// between processes: the file (csrc/ba.hip: /dev/shm/svo_admit_<PCI bus id>) holds 64 slots {pid, admitted workgroups}; a process
// claims a slot (or the slot of a process that no longer exists) and counts the live slots of the others against the same
// budget.  Without the file the admission is per process; a solve that still cannot become co-resident gives up within its bound
// and is re-run (ba_after_giveup), it is never lost.  tests/sanitize/ba_admission_test.cpp walks it on a CPU, across a fork.
#ifndef SVO_BA_ADMISSION_H_
#define SVO_BA_ADMISSION_H_
#include <errno.h>
#include <fcntl.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/types.h>
#include <unistd.h>

#include <atomic>

class BaLedger {
 public:
  const int device;  // whose budget the caller passes to admit()

  // path == null, or a file that cannot be opened, mapped or has no slot left: per process
  BaLedger(const char* path, int device_) : device(device_) {
    const int fd = path ? open(path, O_RDWR | O_CREAT, 0666) : -1;
    if (fd < 0) return;
    if (ftruncate(fd, sizeof(Table)) != 0) { close(fd); return; }
    void* m = mmap(nullptr, sizeof(Table), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return;
    Table* t = static_cast<Table*>(m);
    const int me = (int)getpid();
    for (int pass = 0; pass < 2 && mine_ < 0; ++pass)
      for (int i = 0; i < 64 && mine_ < 0; ++i) {
        int owner = __atomic_load_n(&t->slot[i][0], __ATOMIC_ACQUIRE);
        const bool dead = owner != 0 && owner != me && kill(owner, 0) != 0 && errno == ESRCH;
        if (owner == me || (pass == 1 && (owner == 0 || dead))) {
          if (owner == me || __atomic_compare_exchange_n(&t->slot[i][0], &owner, me, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) {
            __atomic_store_n(&t->slot[i][1], 0, __ATOMIC_RELEASE);
            mine_ = i;
          }
        }
      }
    if (mine_ >= 0) t_ = t; else munmap(m, sizeof(Table));
  }
  ~BaLedger() { if (t_) munmap(t_, sizeof(Table)); }

  bool shared() const { return t_ != nullptr; }
  int admitted() const { return local_.load(std::memory_order_acquire); }                              // by this process
  int published() const { return t_ ? __atomic_load_n(&t_->slot[mine_][1], __ATOMIC_ACQUIRE) : 0; }  // ... as the others see it
  // workgroups the OTHER live processes have admitted on this device
  int others() const {
    if (!t_) return 0;
    int sum = 0;
    for (int i = 0; i < 64; ++i) {
      if (i == mine_) continue;
      const int owner = __atomic_load_n(&t_->slot[i][0], __ATOMIC_ACQUIRE);
      if (owner == 0) continue;
      const int b = __atomic_load_n(&t_->slot[i][1], __ATOMIC_ACQUIRE);
      if (b > 0 && (kill(owner, 0) == 0 || errno != ESRCH)) sum += b;
    }
    return sum;
  }

  bool admit(int n, int budget) {
    if (local_.fetch_add(n, std::memory_order_acq_rel) + n > budget) { local_.fetch_sub(n, std::memory_order_acq_rel); return false; }
    if (t_) {  // publish first, then look at the others: two processes racing may both back off, never both pass
      const int mine_now = __atomic_add_fetch(&t_->slot[mine_][1], n, __ATOMIC_ACQ_REL);
      if (mine_now + others() > budget) {
        __atomic_sub_fetch(&t_->slot[mine_][1], n, __ATOMIC_ACQ_REL);
        local_.fetch_sub(n, std::memory_order_acq_rel);
        return false;
      }
    }
    return true;
  }
  void release(int n) {
    local_.fetch_sub(n, std::memory_order_acq_rel);
    if (t_) __atomic_sub_fetch(&t_->slot[mine_][1], n, __ATOMIC_ACQ_REL);
  }

 private:
  struct Table { int magic; int pad; int slot[64][2]; };
  std::atomic<int> local_{0};
  Table* t_ = nullptr;
  int mine_ = -1;
};

// What one adjuster holds of a ledger for the duration of a solve.
class BaAdmission {
 public:
  bool admit(BaLedger& l, int n, int budget) {
    if (!l.admit(n, budget)) return false;
    ledger_ = &l; blocks_ = n;
    return true;
  }
  void release() { if (blocks_) ledger_->release(blocks_); blocks_ = 0; }
  int blocks() const { return blocks_; }
  ~BaAdmission() { release(); }

 private:
  BaLedger* ledger_ = nullptr;
  int blocks_ = 0;
};

#endif
