"""The random-ops corpus of tests/test_gpu_subopts.py, generated without an
engine so that tests/test_subopts.py can check on the CPU that the reference
restatement alone shows every outcome of run_dispatch_steps/3.

Setup as test_gpu_dispatch.test_dispatch_random_ops_vs_oracle: a 60-filter
pool, 600 steps, a check every 150.  Adds carry random option words; a third
of the subscribers (ids divisible by 3) are only ever added without options.
"""
import random

DESTS = ["n1", "n2", ("g1", "n1"), ("g1", "n2"), ("g2", "n2"), "n3", ("a", "n3"), "g1"]
GROUPS = ["g1", "g2", "g3"]
N_SUBS = 40
SEED = 4177
OUTCOMES = ("dropped", "downgraded", "upgraded", "retain_cleared", "retain_forced", "subid", "no_entry")


def pool(rng, k):
    words = [b"a", b"b", b"", b"+", b"#", b"$SYS", b"c", b"d"]
    out = set()
    while len(out) < k:
        ws = [rng.choice(words) for _ in range(rng.randint(1, 5))]
        if b"#" in ws[:-1]:
            continue
        out.add(b"/".join(ws))
    return sorted(out)


def topics(rng, k):
    words = [b"a", b"b", b"", b"$SYS", b"c", b"d", b"x"]
    return [b"/".join(rng.choice(words) for _ in range(rng.randint(1, 6))) for _ in range(k)]


def rand_opts(rng):
    o = {"qos": rng.randrange(3), "nl": rng.randrange(2), "rap": rng.randrange(2)}
    if rng.random() < 0.4:
        o["subid"] = rng.choice([1, 17, 4096, (1 << 28) - 1])
    return o


def rand_msgs(rng, k):
    """(qos, retain, retained, from): from drawn from the subscriber range, None now and then"""
    return [(rng.randrange(3), rng.randrange(2), 1 if rng.random() < 0.2 else 0,
             None if rng.random() < 0.2 else rng.randrange(N_SUBS)) for _ in range(k)]


def corpus(seed=SEED, reps=2):
    """-> [rep] of [step]: ("route_add" | "route_del", topic, dest), ("add", topic,
    sub, group, opts | None), ("del", topic, sub, group), ("set", topic, sub,
    opts) and ("check", topics, msgs)"""
    rng = random.Random(seed)
    out = []
    for _ in range(reps):
        p = pool(rng, 60)
        steps = []
        for step in range(600):
            t = rng.choice(p)
            x = rng.random()
            if x < 0.4:
                steps.append(("route_add" if rng.random() < 0.7 else "route_del", t, rng.choice(DESTS)))
            else:
                s = rng.randrange(N_SUBS)
                g = rng.choice(GROUPS) if rng.random() < 1 / 3 else None
                y = rng.random()
                if y < 0.65:
                    steps.append(("add", t, s, g, None if s % 3 == 0 else rand_opts(rng)))
                elif y < 0.85:
                    steps.append(("del", t, s, g))
                else:
                    o = rand_opts(rng)
                    steps.append(("set", t, s, {k: o[k] for k in rng.sample(sorted(o), rng.randint(1, len(o)))}))
            if step % 150 == 149:
                tp = topics(rng, 300) + p
                steps.append(("check", tp, rand_msgs(rng, len(tp))))
        out.append(steps)
    return out


def outcomes(opts, msg, result):
    """which of OUTCOMES one pair shows: opts = the option entry (None: none),
    result = run_dispatch_steps' value"""
    if opts is None:
        return {"no_entry"}
    if result is None:
        return {"dropped"}
    seen = set()
    if result[0] < msg[0]:
        seen.add("downgraded")
    if result[0] > msg[0]:
        seen.add("upgraded")
    if msg[1] and not result[1]:
        seen.add("retain_cleared")
    if not msg[1] and msg[2] and result[1]:
        seen.add("retain_forced")
    if result[2] is not None:
        seen.add("subid")
    return seen


def apply_ref(step, table, ref):
    """one non-check step on the oracle's route table and the SubOptionTable"""
    op = step[0]
    if op == "route_add":
        table.add_route(step[1], step[2])
    elif op == "route_del":
        table.del_route(step[1], step[2])
    elif op == "add":
        _, t, s, g, o = step
        if o is None:
            ref.bag.insert_subscriber(g, t, s)
        else:
            ref.do_subscribe(g, t, s, o)
    elif op == "del":
        return ref.do_unsubscribe(step[3], step[1], step[2])
    elif op == "set":
        return ref.set_subopts(step[1], step[2], step[3])
    else:
        raise AssertionError(op)
    return None
