"""Cases of the derived strata's text (include/vcfdist_derive.h): expressions with the parse they must get, crosses with their
pairs, every malformed entry with its message, and random expressions and programs.  The names are the defaults of --stratify-context
and --stratify-variants, in table order, so the same entries go to the library and to both command lines."""
import numpy as np

CONTEXT = ["hp_4to6", "hp_7to11", "hp_ge12", "tr_di_ge10", "tr_tri_ge14", "tr_quad_ge19", "gc_lt25", "gc_25to30", "gc_30to55", "gc_55to65", "gc_ge65"]
VARIANT = ["snp_ti", "snp_tv", "ins_1to5", "ins_6to15", "ins_16to49", "ins_ge50", "del_1to5", "del_6to15", "del_16to49", "del_ge50", "hom", "het",
           "iso_50", "near_10"]
NAMES = CONTEXT + VARIANT
K = {n: k for k, n in enumerate(NAMES)}
AND, OR, NOT = -1, -2, -3


def union_code(ks):
    """the left-associated union of the strata ks"""
    code = []
    for i, k in enumerate(ks):
        code += [k] + ([OR] if i else [])
    return code


# (entry, the same expression fully parenthesised and without globs, the program the library must emit)
h, t, e, m = K["hp_ge12"], K["snp_ti"], K["het"], K["hom"]
PARSES = [
    ("x=hom|het&snp_ti", "(hom|(het&snp_ti))", [m, e, t, AND, OR]),                       # & binds tighter than |
    ("x=hom&het|snp_ti", "((hom&het)|snp_ti)", [m, e, AND, t, OR]),
    ("x=!hom&het", "((!hom)&het)", [m, NOT, e, AND]),                                     # ! binds tighter than &
    ("x=!hom|het", "((!hom)|het)", [m, NOT, e, OR]),
    ("x=!!hom", "(!(!hom))", [m, NOT, NOT]),
    ("x=!(hom&het)", "(!(hom&het))", [m, e, AND, NOT]),
    ("x=hom|het|snp_ti", "((hom|het)|snp_ti)", [m, e, OR, t, OR]),                        # left-associated
    ("x=hom&(het|(snp_ti&!(hp_ge12|hom)))", "(hom&(het|(snp_ti&(!(hp_ge12|hom)))))", [m, e, t, h, m, OR, NOT, AND, OR, AND]),
    ("x=((((hom))))", "hom", [m]),
    ("x= \thom \t& ! ( het\t|snp_ti ) ", "(hom&(!(het|snp_ti)))", [m, e, t, OR, NOT, AND]),   # blanks and tabs between tokens
    (" x\t=hom", "hom", [m]),                                                             # ... and around the name
    ("x=*", "(" + "|".join(NAMES) + ")", union_code(range(len(NAMES)))),
    ("x=hp_*", "(hp_4to6|hp_7to11|hp_ge12)", union_code([0, 1, 2])),
    ("x=*_ge*", "(" + "|".join(n for n in NAMES if "_ge" in n) + ")", union_code([k for k, n in enumerate(NAMES) if "_ge" in n])),
    ("x=!*", "(!(" + "|".join(NAMES) + "))", union_code(range(len(NAMES))) + [NOT]),
    ("x=del_1to5&hp_*", "(del_1to5&(hp_4to6|hp_7to11|hp_ge12))", [K["del_1to5"]] + union_code([0, 1, 2]) + [AND]),
    ("x=h*2", "hp_ge12", [h]),                                                            # a '*' inside, one match
    ("x=**hom**", "hom", [m]),                                                            # a '*' matches the empty run
    ("A.b+c-9_=hom", "hom", [m]),                                                         # every character a name may hold
]
# entries of one command line, in order: a glob takes in the derived names in front of it, and only those
SEQUENCE = ["hp_long=hp_ge12|hp_7to11", "easy=!*", "hp_all=hp_*", "x2=!easy&hp_long", "any=*"]
SEQUENCE_EQUIV = ["(hp_ge12|hp_7to11)", "(!(" + "|".join(NAMES + ["hp_long"]) + "))", "(hp_4to6|hp_7to11|hp_ge12|hp_long)", "((!easy)&hp_long)",
                  "(" + "|".join(NAMES + ["hp_long", "easy", "hp_all", "x2"]) + ")"]

# (entry, its pairs as names)
CROSSES = [
    ("hom:het", [("hom", "het")]),
    ("hom,het:hom,het", [("hom", "het"), ("het", "hom")]),                                # a != b
    ("het,hom:snp_ti", [("hom", "snp_ti"), ("het", "snp_ti")]),                           # table order, not the list's
    ("hom,hom,ho*:snp_t*", [("hom", "snp_ti"), ("hom", "snp_tv")]),                       # each once
    (" hom , het : snp_ti ", [("hom", "snp_ti"), ("het", "snp_ti")]),
    ("ins_*,del_*:hp_*", [(a, b) for a in VARIANT[2:10] for b in CONTEXT[:3]]),           # left-major
]

U = " (an entry names the strata in front of it)"
DEEP = "x=" + "(" * 33 + "hom" + ")" * 33
STACK33 = "x=" + "hom|(" * 32 + "hom" + ")" * 32                                         # parentheses 32 deep, a stack of 33
STACK32 = "x=" + "hom|(" * 31 + "hom" + ")" * 31                                         # the limit itself: valid
LONG = "x=" + "!" * 65536 + "hom"                                                         # 65537 ints of code
# (entry, the message behind "entry '<entry>': ")
MALFORMED = [
    ("hom", "missing '=' (an entry is NAME=EXPR)"), ("", "missing '=' (an entry is NAME=EXPR)"),
    ("=hom", "empty name"), (" \t=hom", "empty name"),
    ("a b=hom", "bad name 'a b' (a name is [A-Za-z0-9_.+-]+)"), ("x&y=hom", "bad name 'x&y' (a name is [A-Za-z0-9_.+-]+)"),
    ("x*=hom", "bad name 'x*' (a name is [A-Za-z0-9_.+-]+)"), ("(x)=hom", "bad name '(x)' (a name is [A-Za-z0-9_.+-]+)"),
    ("hom=het", "name 'hom' is already a stratum"), ("hp_ge12=hp_ge12", "name 'hp_ge12' is already a stratum"),
    ("x=", "empty expression"), ("x= \t", "empty expression"),
    ("x=nosuch", "unknown stratum 'nosuch'" + U), ("x=hom&Hom", "unknown stratum 'Hom'" + U), ("x=hom|hp_ge", "unknown stratum 'hp_ge'" + U),
    ("x=x", "'x' is the entry itself"), ("x=hom|!x", "'x' is the entry itself"),
    ("x=zz*", "glob 'zz*' matches no stratum in front of the entry"), ("x=hom&*_lt5*", "glob '*_lt5*' matches no stratum in front of the entry"),
    ("x=(hom", "unbalanced parenthesis: a '(' is never closed"), ("x=(hom|(het)", "unbalanced parenthesis: a '(' is never closed"),
    ("x=(", "unbalanced parenthesis: a '(' is never closed"),
    ("x=hom)", "unbalanced parenthesis: a ')' closes nothing"), ("x=(hom|het))", "unbalanced parenthesis: a ')' closes nothing"),
    ("x=)", "unbalanced parenthesis: a ')' closes nothing"),
    ("x=hom&", "dangling operator '&'"), ("x=|hom", "dangling operator '|'"), ("x=hom&|het", "dangling operator '|'"), ("x=!", "dangling operator '!'"),
    ("x=hom|!", "dangling operator '!'"), ("x=(hom&)", "dangling operator '&'"), ("x=hom| ", "dangling operator '|'"), ("x=&", "dangling operator '&'"),
    ("x=()", "empty parentheses"),
    ("x=hom het", "missing operator in front of 'het'"), ("x=hom(het)", "missing operator in front of '('"), ("x=hom!het", "missing operator in front of '!'"),
    ("x=hom=het", "unexpected character '=' in the expression"), ("x=hom,het", "unexpected character ',' in the expression"),
    ("x=hom:het", "unexpected character ':' in the expression"), ("x=,", "unexpected character ',' in the expression"),
    (DEEP, "nesting deeper than 32"), (STACK33, "nesting deeper than 32"),
    (LONG, "code longer than 65536"),
]
MALFORMED_CROSS = [
    ("hom", "missing ':' (an entry is LIST:LIST)"), ("", "missing ':' (an entry is LIST:LIST)"), ("hom:het:snp_ti", "more than one ':'"),
    (":hom", "empty left side"), ("hom:", "empty right side"), ("hom: \t", "empty right side"), (":", "empty left side"),
    ("hom,,het:snp_ti", "empty glob on the left side"), ("hom:het,", "empty glob on the right side"),
    ("hom:nosuch", "unknown stratum 'nosuch'" + U), ("zz*:hom", "glob 'zz*' matches no stratum in front of the entry"),
    ("hom:hom", "the cross yields no pair"), ("ho*:h*m", "the cross yields no pair"),
    ("hom&het:snp_ti", "unexpected character '&' in 'hom&het'"), ("hom:(het)", "unexpected character '(' in '(het)'"),
    ("hom:x=het", "unexpected character '=' in 'x=het'"),
]


def random_members(n_strata, n_var, seed):
    """member[n_strata][n_var] with strata of every density, an empty and a full one among them"""
    rng = np.random.RandomState(seed)
    mem = rng.random_sample((n_strata, n_var)) < rng.random_sample((n_strata, 1))
    if n_strata > 2:
        mem[rng.randint(n_strata)] = False
        mem[rng.randint(n_strata)] = True
    return mem


def random_expression(rng, names, depth=0):
    """a random well-formed EXPR over names, with blanks, redundant parentheses and now and then a glob"""
    r = rng.random_sample()
    sp = lambda: " " * rng.randint(0, 2)
    if depth >= 5 or r < 0.3:
        n = names[rng.randint(len(names))]
        if rng.random_sample() < 0.15 and len(n) > 2:
            n = n[:rng.randint(1, len(n))] + "*"
        return sp() + n + sp()
    if r < 0.45:
        return sp() + "!" + random_expression(rng, names, depth + 1)
    if r < 0.6:
        return sp() + "(" + random_expression(rng, names, depth + 1) + ")" + sp()
    return random_expression(rng, names, depth + 1) + "&|"[rng.randint(2)] + random_expression(rng, names, depth + 1)


def random_program(rng, n_front, max_depth=32, steps=None):
    """a random valid program over the strata 0 .. n_front - 1 that reaches a stack of max_depth now and then"""
    code, depth = [], 0
    steps = rng.randint(1, 80) if steps is None else steps
    for _ in range(steps):
        r = rng.random_sample()
        if depth == 0 or (depth < max_depth and r < 0.45):
            code.append(int(rng.randint(n_front))); depth += 1
        elif depth >= 2 and r < 0.8:
            code.append((AND, OR)[rng.randint(2)]); depth -= 1
        else:
            code.append(NOT)
    while depth > 1:
        code.append((AND, OR)[rng.randint(2)]); depth -= 1
    return code


def deep_program(rng, n_front, depth=32):
    """a program whose stack reaches `depth` exactly: `depth` pushes, with NOTs between them, then the folds"""
    code = []
    for _ in range(depth):
        code.append(int(rng.randint(n_front)))
        if rng.random_sample() < 0.5:
            code.append(NOT)
    for _ in range(depth - 1):
        code.append((AND, OR)[rng.randint(2)])
        if rng.random_sample() < 0.3:
            code.append(NOT)
    return code
