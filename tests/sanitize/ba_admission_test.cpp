// The admission ledger (stereo_vo_amd/host/ba_admission.h) walked on the host, under ASan + UBSan; the table file sits in the
// directory given on the command line:
//   * admit up to the budget, one more is refused and leaves both counters (the process's, its published slot) unchanged;
//     release restores the counts, a handle's destructor releases;
//   * a forked child (a process of its own: its own ledger on the same file) admits n: the parent sees n counted against its
//     budget and is refused beyond it, again with both counters unchanged;
//   * the child exits without releasing: its slot no longer counts, and a new process claims that very slot;
//   * without a file (an unwritable path, no path) the admission is per process.
#include <stdio.h>
#include <string.h>
#include <sys/wait.h>

#include <string>

#include "ba_admission.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Child { pid_t pid; int to_child, from_child; };

// A child process with its own ledger on `path` that admits n of `budget`, reports 'y' / 'n', waits for a byte and leaves WITHOUT
// releasing (no destructor runs).
static Child start_child(const char* path, int n, int budget) {
  int down[2], up[2];
  if (pipe(down) || pipe(up)) { perror("pipe"); _exit(2); }
  const pid_t pid = fork();
  if (pid < 0) { perror("fork"); _exit(2); }
  if (pid == 0) {
    alarm(30);  // never outlive a parent that failed
    close(down[1]); close(up[0]);
    BaLedger mine(path, 0);
    BaAdmission hold;
    char c = mine.shared() && hold.admit(mine, n, budget) && mine.published() == n ? 'y' : 'n';
    if (write(up[1], &c, 1) != 1) _exit(3);
    if (read(down[0], &c, 1) < 0) _exit(3);
    _exit(0);
  }
  close(down[0]); close(up[1]);
  return {pid, down[1], up[0]};
}
static bool child_says_yes(const Child& c) { char b = 0; return read(c.from_child, &b, 1) == 1 && b == 'y'; }
static void end_child(const Child& c) {
  char b = 0;
  CHECK(write(c.to_child, &b, 1) == 1, "write to the child");
  int st = -1;
  CHECK(waitpid(c.pid, &st, 0) == c.pid && WIFEXITED(st) && WEXITSTATUS(st) == 0, "the child ended with status %d", st);
  close(c.to_child); close(c.from_child);
}

// the table as another process sees it: {magic, pad, 64 x {pid, admitted workgroups}}
static void read_slot(const char* path, int i, int* pid, int* count) {
  int t[2 + 128] = {0};
  FILE* f = fopen(path, "rb");
  CHECK(f && fread(t, sizeof(int), 130, f) == 130, "the table file holds 64 slots");
  if (f) fclose(f);
  *pid = t[2 + 2 * i]; *count = t[2 + 2 * i + 1];
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: ba_admission_test <empty directory>\n"); return 2; }
  alarm(60);
  const std::string file = std::string(argv[1]) + "/svo_admit_test";
  const char* path = file.c_str();
  const int budget = 10;
  {
    BaLedger l(path, 3);
    CHECK(l.shared() && l.device == 3 && l.admitted() == 0 && l.published() == 0 && l.others() == 0, "a fresh ledger");
    // ---- within one process
    BaAdmission a, b, c;
    CHECK(a.admit(l, 6, budget) && l.admitted() == 6 && l.published() == 6 && a.blocks() == 6, "6 of 10");
    CHECK(b.admit(l, 4, budget) && l.admitted() == 10 && l.published() == 10, "up to the budget");
    CHECK(!c.admit(l, 1, budget) && c.blocks() == 0 && l.admitted() == 10 && l.published() == 10, "one more is refused, nothing changes");
    c.release();  // nothing held: nothing happens
    CHECK(l.admitted() == 10 && l.published() == 10, "releasing nothing");
    a.release();
    CHECK(l.admitted() == 4 && l.published() == 4 && a.blocks() == 0, "release gives 6 back");
    a.release();
    CHECK(l.admitted() == 4 && l.published() == 4, "released twice");
    { BaAdmission d; CHECK(d.admit(l, 6, budget) && l.admitted() == 10, "6 again"); }
    CHECK(l.admitted() == 4 && l.published() == 4, "the destructor releases");
    CHECK(!c.admit(l, 7, budget) && c.admit(l, 6, budget), "7 of the 6 left, then 6");
    b.release(); c.release();
    CHECK(l.admitted() == 0 && l.published() == 0, "all released");
    int pid = 0, count = -1;
    read_slot(path, 0, &pid, &count);
    CHECK(pid == (int)getpid() && count == 0, "slot 0 is {%d, %d}", pid, count);
    // ---- a second process admits 7: they count against this one's budget
    const Child k = start_child(path, 7, budget);
    CHECK(child_says_yes(k), "the child was not admitted");
    CHECK(l.others() == 7, "the others hold %d", l.others());
    CHECK(a.admit(l, 3, budget) && l.admitted() == 3 && l.published() == 3, "3 beside the child's 7");
    CHECK(!b.admit(l, 1, budget) && l.admitted() == 3 && l.published() == 3 && l.others() == 7, "one more is refused across processes, nothing changes");
    read_slot(path, 1, &pid, &count);
    CHECK(pid == (int)k.pid && count == 7, "slot 1 is {%d, %d}", pid, count);
    // ---- it exits without releasing: its slot no longer counts, the next process claims it
    end_child(k);
    CHECK(l.others() == 0, "a dead process still holds %d", l.others());
    CHECK(b.admit(l, 7, budget) && l.admitted() == 10, "the dead child's 7 are free again");
    b.release();
    const Child k2 = start_child(path, 2, budget);
    CHECK(child_says_yes(k2), "the second child was not admitted");
    read_slot(path, 1, &pid, &count);
    CHECK(pid == (int)k2.pid && count == 2, "slot 1 is {%d, %d} after a new process claimed it", pid, count);
    CHECK(l.others() == 2 && l.published() == 3, "the others hold %d", l.others());
    end_child(k2);
    read_slot(path, 2, &pid, &count);
    CHECK(pid == 0 && count == 0, "slot 2 is {%d, %d}: never claimed", pid, count);
    a.release();
    CHECK(l.admitted() == 0 && l.published() == 0, "all released");
  }
  // ---- no file: per process
  const std::string nowhere = file + "/not_a_directory/table";  // (the table file is no directory)
  for (const char* p : {nowhere.c_str(), (const char*)nullptr}) {
    BaLedger l(p, 0);
    BaAdmission a, b;
    CHECK(!l.shared() && l.others() == 0 && l.published() == 0, "a ledger without a file is shared");
    CHECK(a.admit(l, budget, budget) && !b.admit(l, 1, budget) && l.admitted() == budget, "per process: up to the budget");
    a.release();
    CHECK(l.admitted() == 0 && b.admit(l, 1, budget), "per process: release");
  }
  if (fails) { fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  printf("ba admission ok\n");
  return 0;
}
