// test_pool_threads.cpp -- the stream-ordered device pool (csrc/pool.hpp) driven from several host
// threads at once, on a simulated device: no GPU, no HIP.  Built with ThreadSanitizer.
//
// test_pool.cpp states the ordering property on one thread.  Here 8 worker threads, each with a
// stream of its own, take blocks of three sizes from ONE pool, queue writes tagged with their
// thread and round (some also on a second stream), and put the blocks back with the streams that
// used them, while a "device" thread retires the queued operations in random stream order.  The
// pool takes its mutex in take / put / order_after and calls the backend outside it; the backend
// here is thread-safe (one device mutex), as the HIP runtime is.
//
// Checked:
//   * the property of test_pool.cpp: per block, no operation of an earlier owner completes after
//     an operation of a later owner (the first of which is the read the taker queues right after
//     the pool's ordering) -- i.e. a block's operations retire in owner order;
//   * a block is never handed to two owners at once, and always has the size that was asked for;
//   * an event is never re-recorded while its previous record is pending;
//   * ThreadSanitizer sees no data race in the pool's own state.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#include "../../lcpc_proof_of_storage_amd/csrc/pool.hpp"

namespace {

constexpr int N_WORKERS = 8;
constexpr int N_EXTRA = 2;                        // streams no worker owns (a communicator's)
constexpr int N_STREAMS = N_WORKERS + N_EXTRA;    // ids 1 .. N_STREAMS; 0 is "none"
constexpr int ROUNDS = 3000;
constexpr size_t SIZES[3] = {256, 4096, 65536};
constexpr size_t BACKLOG_HI = 48, BACKLOG_LO = 16;  // a worker lets the device catch up past HI
constexpr long DEVICE_LAG = 64;  // operations the device stays behind the hosts while none of them waits

[[noreturn]] void die(const char *what) {
  std::fprintf(stderr, "pool threads: %s\n", what);
  std::abort();
}

struct Op {
  enum Kind { WRITE, READ, WAIT } kind = WRITE;
  int block = -1;      // WRITE / READ
  long gen = 0;        // the block's owner generation when the operation was queued
  unsigned tag = 0;    // WRITE: (thread << 24) | round
  int ev_stream = 0;   // WAIT: the stream of the record it waits for ...
  long target = 0;     // ... and how many of that stream's operations the record covers
};

struct Block {
  int size_class = 0;
  long gen = 0;          // current owner generation
  long retired_gen = 0;  // the highest generation an operation on it has completed with
  unsigned mem = 0;      // the last tag written
  bool owned = false;
};

// The simulated device.  Everything below is guarded by mu.
struct Sim {
  std::mutex mu;
  std::condition_variable cv;  // an operation was queued or retired
  std::vector<Op> q[N_STREAMS + 1];
  long done[N_STREAMS + 1] = {};
  struct Rec {
    int stream = 0;
    long target = 0;
  };
  std::vector<Rec> rec{1};  // by event id (0 is "none")
  std::vector<Block> blocks;
  bool stop = false;
  int waiters = 0;  // host threads blocked on the device (sync, drain, a full backlog)
  long queued = 0, retired = 0, violations = 0;

  bool rec_done(int e) const { return rec[e].stream == 0 || done[rec[e].stream] >= rec[e].target; }
  bool ready(int s) const {
    const long i = done[s];
    if (i >= (long)q[s].size()) return false;
    const Op &o = q[s][i];
    return o.kind != Op::WAIT || done[o.ev_stream] >= o.target;
  }
  void retire(int s) {
    const Op &o = q[s][done[s]];
    if (o.kind != Op::WAIT) {
      Block &b = blocks[o.block];
      if (o.gen < b.retired_gen) {
        std::fprintf(stderr, "ordering violated: stream %d's %s of block %d for owner %ld completed after owner %ld's "
                             "(tag %08x over %08x)\n", s, o.kind == Op::WRITE ? "write" : "read", o.block, o.gen,
                     b.retired_gen, o.tag, b.mem);
        violations++;
      }
      b.retired_gen = std::max(b.retired_gen, o.gen);
      if (o.kind == Op::WRITE) b.mem = o.tag;
    }
    done[s]++;
    retired++;
  }
  // the device: retire ready operations, a random stream at a time
  void run(unsigned seed) {
    std::mt19937 rng(seed);
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      int rs[N_STREAMS], n = 0;
      for (int s = 1; s <= N_STREAMS; s++)
        if (ready(s)) rs[n++] = s;
      if (!n && stop) return;
      // late writers are the point: the device runs only when it is DEVICE_LAG operations behind or
      // a host waits for it, so a released block's fence is usually still pending when it is taken
      if (!n || (waiters == 0 && queued - retired <= DEVICE_LAG && !stop)) {
        cv.wait(lk);
        continue;
      }
      const int s = rs[rng() % n];
      for (int k = 1 + rng() % 3; k > 0 && ready(s); k--) retire(s);
      cv.notify_all();
      if (rng() % 4 == 0) {  // let the hosts run ahead
        lk.unlock();
        std::this_thread::yield();
        lk.lock();
      }
    }
  }
  // (host, mu held) queue an operation
  void push(int s, const Op &o) {
    q[s].push_back(o);
    queued++;
    cv.notify_all();
  }
  // (host, lk on mu held) wait for the device
  template <class Pred>
  void host_wait(std::unique_lock<std::mutex> &lk, Pred pred) {
    if (pred()) return;
    waiters++;
    cv.notify_all();
    cv.wait(lk, pred);
    waiters--;
  }
};

struct SimBackend {
  using Stream = int;
  using Event = int;
  Sim *sim;
  Event event_new() {
    std::lock_guard<std::mutex> lk(sim->mu);
    sim->rec.emplace_back();
    return (int)sim->rec.size() - 1;
  }
  void event_free(Event) {}
  bool record(Event e, Stream s) {
    std::lock_guard<std::mutex> lk(sim->mu);
    if (!sim->rec_done(e)) die("an event was re-recorded while its previous record was pending");
    sim->rec[e] = {s, (long)sim->q[s].size()};
    return true;
  }
  bool done(Event e) {
    std::lock_guard<std::mutex> lk(sim->mu);
    return sim->rec_done(e);
  }
  bool wait(Stream s, Event e) {
    std::lock_guard<std::mutex> lk(sim->mu);
    Op o;
    o.kind = Op::WAIT;
    o.ev_stream = sim->rec[e].stream;
    o.target = sim->rec[e].target;
    if (o.ev_stream) sim->push(s, o);
    return true;
  }
  bool sync(Event e) {
    std::unique_lock<std::mutex> lk(sim->mu);
    sim->host_wait(lk, [&] { return sim->rec_done(e); });
    return true;
  }
  void drain(Stream s) {
    std::unique_lock<std::mutex> lk(sim->mu);
    sim->host_wait(lk, [&] { return sim->done[s] >= (long)sim->q[s].size(); });
  }
};

using Pool = lcpc_pool::OrderedPool<SimBackend>;

void worker(int w, Sim &sim, SimBackend &b, Pool &pool, std::atomic<long> &reused) {
  std::mt19937 rng(1000 + w);
  const int mine = w + 1;
  for (int round = 0; round < ROUNDS; round++) {
    const int sc = rng() % 3;
    // one take in eight is a host taker (no stream): ordered on the host, used on `mine` later
    const bool host_take = rng() % 8 == 0;
    void *p = pool.take(SIZES[sc], host_take ? 0 : mine);
    int blk;
    long gen;
    {
      std::lock_guard<std::mutex> lk(sim.mu);
      if (p) {
        blk = (int)(size_t)p - 1;
        Block &bl = sim.blocks[blk];
        if (bl.owned) die("a block was handed to two owners at once");
        if (bl.size_class != sc) die("a block of another size was handed out");
        bl.gen++;
      } else {
        blk = (int)sim.blocks.size();
        sim.blocks.emplace_back();
        sim.blocks[blk].size_class = sc;
      }
      sim.blocks[blk].owned = true;
      gen = sim.blocks[blk].gen;
      // the new owner's first touch: a read right behind the pool's ordering
      Op rd;
      rd.kind = Op::READ;
      rd.block = blk;
      rd.gen = gen;
      sim.push(mine, rd);
    }
    if (p) reused++;
    // the owner's writes, tagged, on its stream -- and for some blocks on a second stream too,
    // ordered after the first use by an event of the owner's (the library's cross-stream events)
    int used[2] = {mine, 0};
    Op wr;
    wr.kind = Op::WRITE;
    wr.block = blk;
    wr.gen = gen;
    wr.tag = (unsigned)w << 24 | (unsigned)round;
    const int n_writes = 1 + rng() % 3;
    {
      std::lock_guard<std::mutex> lk(sim.mu);
      for (int k = 0; k < n_writes; k++) sim.push(mine, wr);
    }
    if (rng() % 3 == 0) {
      int s2 = 1 + rng() % N_STREAMS;  // another worker's stream or a shared one
      if (s2 == mine) s2 = N_WORKERS + 1;
      std::lock_guard<std::mutex> lk(sim.mu);
      Op wt;
      wt.kind = Op::WAIT;
      wt.ev_stream = mine;
      wt.target = (long)sim.q[mine].size();
      sim.push(s2, wt);
      sim.push(s2, wr);
      used[1] = s2;
    }
    {
      std::lock_guard<std::mutex> lk(sim.mu);
      sim.blocks[blk].owned = false;
    }
    pool.put((void *)(size_t)(blk + 1), SIZES[sc], used, used[1] ? 2 : 1);
    // keep a backlog on the device (late writers are the point), but a bounded one
    std::unique_lock<std::mutex> lk(sim.mu);
    if (sim.q[mine].size() - (size_t)sim.done[mine] > BACKLOG_HI)
      sim.host_wait(lk, [&] { return sim.q[mine].size() - (size_t)sim.done[mine] <= BACKLOG_LO; });
  }
}

}  // namespace

int main() {
  Sim sim;
  SimBackend b{&sim};
  long waits = 0, same = 0, syncs = 0;
  std::atomic<long> reused{0};
  {
    Pool pool(b);
    std::thread device([&] { sim.run(7); });
    std::vector<std::thread> ws;
    for (int w = 0; w < N_WORKERS; w++) ws.emplace_back([&, w] { worker(w, sim, b, pool, reused); });
    for (auto &t : ws) t.join();
    for (int s = 1; s <= N_STREAMS; s++) b.drain(s);
    {
      std::lock_guard<std::mutex> lk(sim.mu);
      sim.stop = true;
      sim.cv.notify_all();
    }
    device.join();
    waits = (long)pool.waits_issued();
    same = (long)pool.same_stream();
    syncs = (long)pool.host_syncs();
    size_t freed = 0;
    pool.drain([&](void *) { freed++; });
    if (freed != sim.blocks.size() || pool.cached() != 0) die("blocks were lost or duplicated in the pool");
  }
  std::printf("pool threads: %zu blocks, %ld reused, %ld operations retired, %ld stream waits, %ld own-stream takes, "
              "%ld host waits\n", sim.blocks.size(), reused.load(), sim.retired, waits, same, syncs);
  if (sim.violations) die("ordering violations (above)");
  // the run must have exercised what it is about: blocks recycled between threads behind a wait
  if (reused.load() < N_WORKERS * ROUNDS / 2 || waits == 0 || syncs == 0) die("the run recycled too few blocks to prove anything");
  std::printf("pool threads: ok\n");
  return 0;
}
