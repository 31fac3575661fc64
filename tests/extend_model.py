"""The reference's table extensions restated on Python integers, row by row AS THE REFERENCE WRITES THEM -- loops with `if`s, not scans
with masks: `extend` of processor_table.py:359-427, instruction_table.py:171-231, memory_table.py:174-206 and `extend_iotable` of
io_table.py:77-110.  Nothing here calls the package.  tests/golden/extend.json holds what the reference itself made of the tables of
extend_cases.py; tests/test_extend_host.py checks this module against it, and the package (host and device) against this module.

Cells are integers below p, extension elements triples of limbs.  Every function returns (columns, terminals): per extension column
the list of its values, one triple per row, and the terminals in the order of the columns."""
from scan_model import P, X0, xadd, xmul, xscale, xsub

COMMA, DOT = ord(","), ord(".")
MINUS_ONE = (P - 1, 0, 0)           # `-one`: what the instruction table's loop starts its previous address with


def lift(v):
    return (v, 0, 0)


def processor(matrix, challenges, initials):
    """cycle, instruction pointer, current instruction, next instruction, memory pointer, memory value, inverse"""
    a, b, c, d, e, f, alpha, beta, gamma, delta, eta = challenges
    ipp, mpp = initials
    iev = oev = X0
    cols = ([], [], [], [])
    for i in range(len(matrix)):
        clk, ip, ci, ni, mp, mv, _ = matrix[i]
        cols[0].append(ipp)
        if ci != 0:                                 # not padding
            ipp = xmul(ipp, xsub(xsub(xsub(alpha, xscale(a, ip)), xscale(b, ci)), xscale(c, ni)))
        cols[1].append(mpp)
        if ci != 0:
            mpp = xmul(mpp, xsub(xsub(xsub(beta, xscale(d, clk)), xscale(e, mp)), xscale(f, mv)))
        cols[2].append(iev)
        if ci == COMMA:                             # the input symbol is the NEXT row's memory value (no such row after the last one)
            iev = xadd(xmul(iev, gamma), lift(matrix[i + 1][5]))
        cols[3].append(oev)
        if ci == DOT:
            oev = xadd(xmul(oev, delta), lift(mv))
    return list(cols), [ipp, mpp, iev, oev]


def instruction(matrix, challenges, initials):
    """address, current instruction, next instruction"""
    a, b, c, d, e, f, alpha, beta, gamma, delta, eta = challenges
    product, evaluation = initials[0], X0
    previous_address = MINUS_ONE
    cols = ([], [])
    for i in range(len(matrix)):
        address, ci, ni = matrix[i]
        if ci != 0:
            if i > 0 and address == matrix[i - 1][0]:
                product = xmul(product, xsub(xsub(xsub(alpha, xscale(a, address)), xscale(b, ci)), xscale(c, ni)))
        cols[0].append(product)
        if lift(address) != previous_address:
            evaluation = xadd(xadd(xadd(xmul(eta, evaluation), xscale(a, address)), xscale(b, ci)), xscale(c, ni))
        cols[1].append(evaluation)
        previous_address = lift(address)
    return list(cols), [product, evaluation]


def memory(matrix, challenges, initials):
    """cycle, memory pointer, memory value, dummy"""
    a, b, c, d, e, f, alpha, beta, gamma, delta, eta = challenges
    product = initials[1]
    col = []
    for i in range(len(matrix)):
        clk, mp, mv, dummy = matrix[i]
        col.append(product)
        if dummy == 0:
            product = xmul(product, xsub(xsub(xsub(beta, xscale(d, clk)), xscale(e, mp)), xscale(f, mv)))
    return [col], [product]


def io(matrix, iota, length):
    """one column of symbols; the terminal is the value after row length - 1 (zero for a table of length 0)"""
    evaluation = terminal = X0
    col = []
    for i in range(len(matrix)):
        evaluation = xadd(xmul(evaluation, iota), lift(matrix[i][0]))
        col.append(evaluation)
        if i == length - 1:
            terminal = evaluation
    return [col], [terminal]


def extend(case):
    """a case of extend_cases.py -> (columns, terminals)"""
    table, matrix, challenges, initials = case["table"], case["matrix"], case["challenges"], case["initials"]
    if table == "processor":
        return processor(matrix, challenges, initials)
    if table == "instruction":
        return instruction(matrix, challenges, initials)
    if table == "memory":
        return memory(matrix, challenges, initials)
    return io(matrix, challenges[{"input": 8, "output": 9}[table]], case["length"])
